"""Inputs of tests/test_selection_host.py and tests/test_selection_gpu.py: seeded normal deviates whose every decision
(each row's nearest reference row, each pick of a selection) is clear of rounding, checked here on the CPU, and
brute-force statements of the two definitions of include/rn_select.h in plain loops.  A plain module: no conftest, no
pytest settings."""
import functools

import numpy as np

GAP = 1e-9  # a decision is clear when best and runner-up differ by more than GAP (|x'|^2 + |r'|^2)


def brute_nearest(rows, others, scale=None, exclude_self=False):
    """``(squared distance, index)`` per row, by loops over every pair: the lowest index among equal values."""
    scale = np.ones(rows.shape[1]) if scale is None else scale
    squared, index = np.full(len(rows), np.inf), np.full(len(rows), -1, dtype=np.int64)
    for s, x in enumerate(rows):
        for j, r in enumerate(others):
            if exclude_self and j == s:
                continue
            d2 = float(sum(((a - b) * w) ** 2 for a, b, w in zip(x, r, scale)))
            if index[s] < 0 or d2 < squared[s]:
                squared[s], index[s] = d2, j
    return squared, index


def brute_farthest(rows, count, others=None, first=None, scale=None):
    """``(picks, squared distances)`` by loops: the lowest index among equal values, picked rows last."""
    scale = np.ones(rows.shape[1]) if scale is None else scale
    d2 = lambda a, b: float(sum(((p - q) * w) ** 2 for p, q, w in zip(a, b, scale)))  # noqa: E731
    seeded = others is not None and len(others) > 0
    mind = [min(d2(x, r) for r in others) if seeded else np.inf for x in rows]
    if not seeded and first is None:
        mean = rows.mean(axis=0)
        spread = [d2(x, mean) for x in rows]
        first = spread.index(max(spread))
    picks, squared, picked = [], [], set()
    for k in range(count):
        if k == 0 and not seeded:
            pick = first
        else:
            left = [s for s in range(len(rows)) if s not in picked]
            pick = max(left, key=lambda s: (mind[s], -s))
        picks.append(pick)
        squared.append(mind[pick])
        picked.add(pick)
        mind = [min(m, d2(x, rows[pick])) for m, x in zip(mind, rows)]
    return np.array(picks, dtype=np.int64), np.array(squared)


def _params(columns, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=columns), np.exp(rng.normal(scale=0.5, size=columns))


def _pairwise(rows, others, scale):
    a, b = rows * scale, others * scale
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)


def nearest_gap(rows, others, center, scale, exclude_self=False):
    """The smallest margin of any row, (runner-up - best) / (|x'|^2 + |r'|^2) with r the best row: > GAP is clear."""
    if len(others) - int(exclude_self) < 2:
        return np.inf
    d2 = _pairwise(rows, others, scale)
    if exclude_self:
        d2[np.arange(len(rows)), np.arange(len(rows))] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")
    best, second = order[:, 0], order[:, 1]
    at = np.arange(len(rows))
    norms = (((rows - center) * scale) ** 2).sum(axis=1) + (((others[best] - center) * scale) ** 2).sum(axis=1)
    return float(((d2[at, second] - d2[at, best]) / norms).min())


@functools.lru_cache(maxsize=None)
def nearest_case(rows, references, columns, with_params, seed=20261021):
    """``(X, R, center, scale)`` (the last two ``None`` without params) from the first seed, counting up from ``seed``,
    whose every row has a clear nearest reference row."""
    for attempt in range(seed, seed + 50):
        rng = np.random.default_rng(attempt)
        x, r = rng.normal(size=(rows, columns)), rng.normal(size=(references, columns))
        center, scale = _params(columns, attempt + 1) if with_params else (np.zeros(columns), np.ones(columns))
        if nearest_gap(x, r, center, scale) > GAP:
            return (x, r, center, scale) if with_params else (x, r, None, None)
    raise AssertionError("no seed with a clear nearest row for every row")


def farthest_gap(rows, count, others, first, scale):
    """The smallest margin of any pick, (best - runner-up) / (2 max |x'|^2) over the rows not picked yet."""
    seeded = others is not None and len(others) > 0
    bound = 2.0 * ((rows * scale) ** 2).sum(axis=1).max() + (2.0 * ((others * scale) ** 2).sum(axis=1).max() if seeded else 0.0)
    mind = _pairwise(rows, others, scale).min(axis=1) if seeded else np.full(len(rows), np.inf)
    picked = np.zeros(len(rows), dtype=bool)
    margin = np.inf
    for k in range(count):
        if k == 0 and not seeded:
            values = _pairwise(rows, rows.mean(axis=0)[None], scale)[:, 0]
            forced = first
        else:
            values, forced = np.where(picked, -np.inf, mind), None
        order = np.argsort(-values, kind="stable")
        if forced is None and len(rows) - picked.sum() >= 2:
            margin = min(margin, float((values[order[0]] - values[order[1]]) / bound))
        pick = int(order[0]) if forced is None else forced
        picked[pick] = True
        mind = np.minimum(mind, _pairwise(rows, rows[pick][None], scale)[:, 0])
    return margin


@functools.lru_cache(maxsize=None)
def farthest_case(rows, count, mode, with_params, columns=5, references=40, seed=20261021):
    """``(X, R or None, first or None, scale or None)`` for ``mode`` in ("mean", "first", "reference"), from the first
    seed whose every pick (the default first pick included) is clear."""
    for attempt in range(seed, seed + 50):
        rng = np.random.default_rng(attempt)
        x = rng.normal(size=(rows, columns))
        r = rng.normal(size=(references, columns)) if mode == "reference" else None
        first = rows // 2 if mode == "first" else None
        scale = _params(columns, attempt + 1)[1] if with_params else np.ones(columns)
        if farthest_gap(x, count, r, first, scale) > GAP:
            return x, r, first, scale if with_params else None
    raise AssertionError("no seed with a clear choice at every pick")
