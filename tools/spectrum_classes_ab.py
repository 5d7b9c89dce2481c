#!/usr/bin/env python3
"""A/B of the twenty MD spectrum classes of ramannoodle_amd.spectrum between two trees (profiles/spectrum_classes_ab.txt).

Only the public API is used, so this one file runs unchanged on both trees: --tree names the directory that holds the
ramannoodle_amd package to import (default: this file's repository); RN_POTGNN_LIB selects the library as usual.

  --dump DIR       build every class from seeded inputs at small shapes (33 frames; runs (17, 17) and (33, 21);
                   segment_steps = 9, hop = 4, tapers "hann" and "boxcar"; K = 1 (squeezed) and K = 3; G = 3 groups,
                   C = 4 channels, N = 5 atoms, M = 4 vectors; a fixed and a per-frame lattice; two bands that each hold
                   a bin), call every public measurement with every combination that exists (average, corrections,
                   device=None, device=0, host=True on the device classes, select, measure_interference*, fit_peaks)
                   and a list of refused constructions and calls.  Writes DIR/host.npz and DIR/refused.json, and with a
                   GPU DIR/device.npz: every array under the name of the call that made it, every exception as
                   (type, text).  Prints the SHA-256 of each file's arrays.
  --compare A B [C]  host.npz and refused.json of A and B must be equal byte for byte.  With C, the device rule: A and
                   B are two dumps of the parent, C one of the new tree; where A and B agree byte for byte C must too,
                   and elsewhere C's largest difference from A or B must not exceed that between A and B.  Exit 1 if not.
  --latency        median per-call latency in microseconds of three small device-resident measurements, 500 calls after
                   50 warm-up calls: one JSON line.
"""
import argparse
import dataclasses
import hashlib
import itertools
import json
import os
import sys
import time

import numpy as np

SEED = 20240611
DT = 1.0  # fs: at W = 9 the bins are 4170 cm^-1 apart
W, HOP = 9, 4
W_FIT, HOP_FIT = 17, 8  # fit_peaks: a fit needs at least five bins, segments of 9 frames have three
BANDS = [[3000.0, 5000.0], [7000.0, 13000.0]]
CORRECTIONS = {"raw": {}, "cor": {"laser_correction": True, "bose_einstein_correction": True, "temperature": 250}}
RUN_SETS = {"r17_17": (17, 17), "r33_21": (33, 21)}


# ----------------------------------------------------------------------------- inputs
def inputs():
    rng = np.random.default_rng(SEED)
    data = {"lattice": np.array([[4.1, 0.0, 0.0], [0.3, 3.9, 0.0], [-0.2, 0.4, 4.3]])}
    for name, steps in (("s33", 33), ("r17a", 17), ("r17b", 17), ("r33", 33), ("r21", 21)):
        alpha = rng.normal(size=(steps, 3, 3))
        data[f"alpha_{name}"] = np.ascontiguousarray(alpha + np.swapaxes(alpha, 1, 2)).cumsum(axis=0)
        groups = rng.normal(size=(steps - 1, 3, 3, 3))
        data[f"groups_{name}"] = np.ascontiguousarray(groups + np.swapaxes(groups, 2, 3))
        channels = rng.normal(size=(steps - 1, 4, 3, 3))
        data[f"channels_{name}"] = np.ascontiguousarray(channels + np.swapaxes(channels, 2, 3))
        data[f"positions_{name}"] = 0.02 * rng.normal(size=(steps, 5, 3)).cumsum(axis=0) + rng.random((1, 5, 3))
        data[f"lattices_{name}"] = data["lattice"][None] * (1.0 + 0.01 * rng.normal(size=(steps, 1, 1)))
    data["masses"] = rng.uniform(1.0, 50.0, size=5)
    data["labels"] = np.array([0, 2, 1, 1, 0])
    data["vectors"] = rng.normal(size=(4, 5, 3))
    data["incident"] = rng.normal(size=(3, 3))
    data["scattered"] = rng.normal(size=(3, 3))
    return data


def runs_of(data, kind, run_set):
    names = {"r17_17": ("r17a", "r17b"), "r33_21": ("r33", "r21")}[run_set]
    return [data[f"{kind}_{name}"] for name in names]


# ----------------------------------------------------------------------------- recording
class Record:
    def __init__(self):
        self.arrays, self.refused = {}, []

    def store(self, name, value):
        if dataclasses.is_dataclass(value):
            for field in dataclasses.fields(value):
                self.store(f"{name}.{field.name}", getattr(value, field.name))
        elif isinstance(value, (tuple, list)):
            for index, item in enumerate(value):
                self.store(f"{name}[{index}]", item)
        else:
            if hasattr(value, "detach"):
                value = value.detach().cpu().numpy()
            assert name not in self.arrays, name
            self.arrays[name] = np.array(value)

    def call(self, name, function):
        """Store what ``function()`` returns, or the exception it raises."""
        try:
            value = function()
        except Exception as exc:  # pylint: disable=broad-except
            self.refused.append([name, type(exc).__name__, str(exc)])
            return None
        self.store(name, value)
        return value


def device_options(on_device: bool, gpu: bool):
    """The ``device=`` / ``host=`` combinations a class has: ``(tag, keywords, touches the GPU)``."""
    if on_device:
        return [("dev_default", {}, True), ("dev0", {"device": 0}, True), ("host", {"host": True}, False)]
    return [("host", {}, False)] + ([("dev0", {"device": 0}, True)] if gpu else [])


def polarizations(data):
    return {"k1": (data["incident"][0], data["scattered"][0], None),
            "k3": (data["incident"], data["scattered"], "polycrystalline"),
            "k3r": (data["incident"], data["scattered"][1], np.eye(3)[[1, 2, 0]])}


def measure_raman(record, name, spectrum, data, options):
    """Every weight-contracted measurement of a whole, partial or mode Raman class."""
    record.call(f"{name}.segment_starts", lambda: spectrum.segment_starts(W, HOP))
    record.call(f"{name}.segment_starts_default_hop", lambda: spectrum.segment_starts(W))
    for (tag, where, _), (ctag, cor) in itertools.product(options, CORRECTIONS.items()):
        key = f"{name}.{tag}.{ctag}"
        record.call(f"{key}.measure", lambda: spectrum.measure(**cor, **where))
        for ptag, (e_i, e_s, orientation) in polarizations(data).items():
            record.call(f"{key}.measure_polarized.{ptag}",
                        lambda: spectrum.measure_polarized(e_i, e_s, orientation, **cor, **where))
        for taper, average in itertools.product(("hann", "boxcar"), (True, False)):
            skey = f"{key}.{taper}.{'mean' if average else 'rows'}"
            record.call(f"{skey}.measure_segments",
                        lambda: spectrum.measure_segments(W, HOP, taper, average, **cor, **where))
            for ptag, (e_i, e_s, orientation) in polarizations(data).items():
                record.call(f"{skey}.measure_segments_polarized.{ptag}",
                            lambda: spectrum.measure_segments_polarized(e_i, e_s, orientation, segment_steps=W, hop=HOP,
                                                                        taper=taper, average=average, **cor, **where))
    tag, where, _ = options[0]
    record.call(f"{name}.{tag}.not_polycrystalline", lambda: spectrum.measure(orientation=np.eye(3), **where))
    record.call(f"{name}.{tag}.segments_too_long", lambda: spectrum.measure_segments(40, **where))
    record.call(f"{name}.{tag}.hann_at_three", lambda: spectrum.measure_segments(3, 1, "hann", **where))
    record.call(f"{name}.{tag}.whole_as_segment", lambda: spectrum.measure_segments(17, 17, "boxcar", **where))


def measure_interference(record, name, spectrum, data, options):
    for (tag, where, _), (ctag, cor) in itertools.product(options, CORRECTIONS.items()):
        for stag, segments in (("whole", {}), ("hann", {"segment_steps": W, "hop": HOP}),
                               ("boxcar", {"segment_steps": W, "hop": HOP, "taper": "boxcar"})):
            key = f"{name}.{tag}.{ctag}.{stag}"
            record.call(f"{key}.measure_interference",
                        lambda: spectrum.measure_interference(BANDS, **segments, **cor, **where))
            for ptag, (e_i, e_s, orientation) in polarizations(data).items():
                record.call(f"{key}.measure_interference_polarized.{ptag}",
                            lambda: spectrum.measure_interference_polarized(e_i, e_s, orientation, bands=BANDS,
                                                                            **segments, **cor, **where))
    tag, where, _ = options[0]
    record.call(f"{name}.{tag}.band_without_bin",
                lambda: spectrum.measure_interference([[100.0, 200.0]], segment_steps=W, **where))
    record.call(f"{name}.{tag}.band_empty", lambda: spectrum.measure_interference([[300.0, 200.0]], **where))
    record.call(f"{name}.{tag}.bands_shape", lambda: spectrum.measure_interference([100.0, 200.0], **where))


def measure_select(record, name, spectrum, data, options):
    for ctag, channels in (("c2_0", [2, 0]), ("c1", [1])):
        chosen = record_object(record, f"{name}.select.{ctag}", lambda: spectrum.select(channels))
        if chosen is None:
            continue
        for tag, where, _ in options:
            record.call(f"{name}.select.{ctag}.{tag}.measure", lambda: chosen.measure(**where))
            record.call(f"{name}.select.{ctag}.{tag}.measure_segments",
                        lambda: chosen.measure_segments(W, HOP, "hann", False, **where))
    record.call(f"{name}.select.out_of_range", lambda: type(spectrum.select([0, 4])).__name__)
    record.call(f"{name}.select.negative", lambda: type(spectrum.select([-1])).__name__)
    record.call(f"{name}.select.repeated", lambda: type(spectrum.select([1, 1])).__name__)
    record.call(f"{name}.select.none", lambda: type(spectrum.select([])).__name__)
    record.call(f"{name}.select.floats", lambda: type(spectrum.select([0.0])).__name__)


def measure_vdos(record, name, vdos, options, modes: bool):
    record.call(f"{name}.segment_starts", lambda: vdos.segment_starts(W, HOP))
    for tag, where, touches in options:
        key = f"{name}.{tag}"
        record.call(f"{key}.measure", lambda: vdos.measure(**where))
        for taper, average in itertools.product(("hann", "boxcar"), (True, False)):
            skey = f"{key}.{taper}.{'mean' if average else 'rows'}"
            record.call(f"{skey}.measure_segments", lambda: vdos.measure_segments(W, HOP, taper, average, **where))
            if modes:
                centres = np.array([4170.0, 8340.0, 8340.0, 12500.0])
                record.call(f"{skey}.fit_peaks",
                            lambda: vdos.fit_peaks(centres, 9000.0, W_FIT, HOP_FIT, taper, average, **where))
                if touches:
                    record.call(f"{skey}.fit_peaks_fit0",
                                lambda: vdos.fit_peaks(centres, 9000.0, W_FIT, HOP_FIT, taper, average, fit_device=0,
                                                       **where))
        if modes:
            centres = np.array([5000.0, 8000.0, 9000.0, 11000.0])
            record.call(f"{key}.fit_peaks_whole", lambda: vdos.fit_peaks(centres, 6000.0, **where))
            record.call(f"{key}.fit_peaks_wrong_count", lambda: vdos.fit_peaks(centres[:3], 6000.0, **where))
    tag, where, _ = options[0]
    record.call(f"{name}.{tag}.segments_too_long", lambda: vdos.measure_segments(40, **where))


def record_object(record, name, build):
    """Build an object; record its class name and public properties, or why it was refused."""
    try:
        made = build()
    except Exception as exc:  # pylint: disable=broad-except
        record.refused.append([name, type(exc).__name__, str(exc)])
        return None
    record.store(f"{name}.class", np.array(type(made).__name__))
    for attribute in ("polarizability_ts", "increments", "positions_ts", "timestep", "run_lengths", "runs", "num_groups",
                      "num_channels", "num_modes", "vectors"):
        if hasattr(type(made), attribute):
            record.call(f"{name}.{attribute}", lambda: getattr(made, attribute))
    return made


# ----------------------------------------------------------------------------- the twenty classes
def exercise(record, spectrum, data, gpu: bool, device_pass: bool):
    """``device_pass`` False: the host classes on their host paths (what a machine without a GPU can run, and what must
    be byte for byte across trees).  True: every path that touches the GPU, host classes with ``device=0`` included."""
    import torch
    s = spectrum

    def tensor(array):
        return torch.tensor(np.ascontiguousarray(array), dtype=torch.float64, device="cuda:0")

    host = [option for option in device_options(False, gpu) if option[2] == device_pass]
    resident = device_options(True, gpu) if device_pass else []
    lattices = {"fixed": lambda name: data["lattice"], "perframe": lambda name: data[f"lattices_{name}"]}

    # single runs ---------------------------------------------------------------------------------------------------
    if host:
        made = record_object(record, "MDRamanSpectrum", lambda: s.MDRamanSpectrum(data["alpha_s33"], DT))
        measure_raman(record, "MDRamanSpectrum", made, data, host)
        made = record_object(record, "PartialMDRamanSpectrum", lambda: s.PartialMDRamanSpectrum(data["groups_s33"], DT))
        measure_raman(record, "PartialMDRamanSpectrum", made, data, host)
        made = record_object(record, "ModeMDRamanSpectrum", lambda: s.ModeMDRamanSpectrum(data["channels_s33"], DT))
        measure_raman(record, "ModeMDRamanSpectrum", made, data, host)
        measure_interference(record, "ModeMDRamanSpectrum", made, data, host)
        measure_select(record, "ModeMDRamanSpectrum", made, data, host)
        for ltag, lattice in lattices.items():
            name = f"VibrationalDensityOfStates.{ltag}"
            made = record_object(record, name, lambda: s.VibrationalDensityOfStates(
                data["positions_s33"], DT, lattice("s33"), data["masses"], data["labels"], 3))
            measure_vdos(record, name, made, host, False)
            name = f"ModeVibrationalDensityOfStates.{ltag}"
            made = record_object(record, name, lambda: s.ModeVibrationalDensityOfStates(
                data["positions_s33"], DT, lattice("s33"), data["vectors"], data["masses"]))
            measure_vdos(record, name, made, host, True)
    if resident:
        made = record_object(record, "DeviceMDRamanSpectrum", lambda: s.DeviceMDRamanSpectrum(tensor(data["alpha_s33"]), DT))
        measure_raman(record, "DeviceMDRamanSpectrum", made, data, resident)
        made = record_object(record, "DevicePartialMDRamanSpectrum",
                             lambda: s.DevicePartialMDRamanSpectrum(tensor(data["groups_s33"]), DT))
        measure_raman(record, "DevicePartialMDRamanSpectrum", made, data, resident)
        made = record_object(record, "DeviceModeMDRamanSpectrum",
                             lambda: s.DeviceModeMDRamanSpectrum(tensor(data["channels_s33"]), DT))
        measure_raman(record, "DeviceModeMDRamanSpectrum", made, data, resident)
        measure_interference(record, "DeviceModeMDRamanSpectrum", made, data, resident)
        measure_select(record, "DeviceModeMDRamanSpectrum", made, data, resident)
        for (ltag, lattice), lattice_on_device in itertools.product(lattices.items(), (False, True)):
            where = "_tensor" if lattice_on_device else ""
            place = tensor if lattice_on_device else (lambda array: array)
            name = f"DeviceVibrationalDensityOfStates.{ltag}{where}"
            made = record_object(record, name, lambda: s.DeviceVibrationalDensityOfStates(
                tensor(data["positions_s33"]), DT, place(lattice("s33")), data["masses"], data["labels"], 3))
            measure_vdos(record, name, made, resident, False)
            name = f"DeviceModeVibrationalDensityOfStates.{ltag}{where}"
            made = record_object(record, name, lambda: s.DeviceModeVibrationalDensityOfStates(
                tensor(data["positions_s33"]), DT, place(lattice("s33")), data["vectors"], data["masses"]))
            measure_vdos(record, name, made, resident, True)

    # ensembles -----------------------------------------------------------------------------------------------------
    for run_set in RUN_SETS:
        alpha, groups, channels, positions, per_run = (runs_of(data, kind, run_set) for kind in
                                                       ("alpha", "groups", "channels", "positions", "lattices"))
        run_lattices = {"fixed": data["lattice"], "perframe": per_run}
        if host:
            name = f"MDRamanEnsemble.{run_set}"
            made = record_object(record, name, lambda: s.MDRamanEnsemble(alpha, DT))
            measure_raman(record, name, made, data, host)
            name = f"PartialMDRamanEnsemble.{run_set}"
            made = record_object(record, name, lambda: s.PartialMDRamanEnsemble(groups, DT))
            measure_raman(record, name, made, data, host)
            name = f"ModeMDRamanEnsemble.{run_set}"
            made = record_object(record, name, lambda: s.ModeMDRamanEnsemble(channels, DT))
            measure_raman(record, name, made, data, host)
            measure_interference(record, name, made, data, host)
            measure_select(record, name, made, data, host)
            for ltag, lattice in run_lattices.items():
                name = f"VibrationalDensityOfStatesEnsemble.{run_set}.{ltag}"
                made = record_object(record, name, lambda: s.VibrationalDensityOfStatesEnsemble(
                    positions, DT, lattice, data["masses"], data["labels"], 3))
                measure_vdos(record, name, made, host, False)
                name = f"ModeVibrationalDensityOfStatesEnsemble.{run_set}.{ltag}"
                made = record_object(record, name, lambda: s.ModeVibrationalDensityOfStatesEnsemble(
                    positions, DT, lattice, data["vectors"], data["masses"]))
                measure_vdos(record, name, made, host, True)
        if not resident:
            continue
        frames = [len(run) for run in alpha]
        for form in ("sequence", "joined"):
            def rows(parts, gap: bool):
                """The constructor's ``(runs, run_lengths)`` arguments in this form."""
                if form == "sequence":
                    return [tensor(part) for part in parts], {}
                if gap:  # a batched evaluation writes some row where the zero row would stand
                    filler = np.full((1, *parts[0].shape[1:]), 7.0)
                    parts = [piece for part in parts for piece in (part, filler)][:-1]
                return tensor(np.concatenate(parts)), {"run_lengths": frames}
            name = f"DeviceMDRamanEnsemble.{run_set}.{form}"
            made = record_object(record, name,
                                 lambda: (lambda a, k: s.DeviceMDRamanEnsemble(a, DT, **k))(*rows(alpha, False)))
            measure_raman(record, name, made, data, resident)
            name = f"DevicePartialMDRamanEnsemble.{run_set}.{form}"
            made = record_object(record, name,
                                 lambda: (lambda a, k: s.DevicePartialMDRamanEnsemble(a, DT, **k))(*rows(groups, True)))
            measure_raman(record, name, made, data, resident)
            name = f"DeviceModeMDRamanEnsemble.{run_set}.{form}"
            made = record_object(record, name,
                                 lambda: (lambda a, k: s.DeviceModeMDRamanEnsemble(a, DT, **k))(*rows(channels, True)))
            measure_raman(record, name, made, data, resident)
            measure_interference(record, name, made, data, resident)
            measure_select(record, name, made, data, resident)
            for ltag, lattice in (("fixed", data["lattice"]), ("perframe", np.concatenate(per_run)),
                                  ("perframe_tensor", tensor(np.concatenate(per_run)))):
                name = f"DeviceVibrationalDensityOfStatesEnsemble.{run_set}.{form}.{ltag}"
                made = record_object(record, name, lambda: (lambda a, k: s.DeviceVibrationalDensityOfStatesEnsemble(
                    a, DT, lattice, data["masses"], data["labels"], 3, **k))(*rows(positions, False)))
                measure_vdos(record, name, made, resident, False)
                name = f"DeviceModeVibrationalDensityOfStatesEnsemble.{run_set}.{form}.{ltag}"
                made = record_object(record, name, lambda: (lambda a, k: s.DeviceModeVibrationalDensityOfStatesEnsemble(
                    a, DT, lattice, data["vectors"], data["masses"], **k))(*rows(positions, False)))
                measure_vdos(record, name, made, resident, True)


def refusals(record, spectrum, data, gpu: bool):
    """Constructions and calls that must be refused, with the same type and text in both trees."""
    s = spectrum
    a, g, c, p = data["alpha_s33"], data["groups_s33"], data["channels_s33"], data["positions_s33"]
    lattice, masses, vectors = data["lattice"], data["masses"], data["vectors"]
    cases = {
        "MDRamanSpectrum.shape": lambda: s.MDRamanSpectrum(a[:, :2], DT),
        "MDRamanSpectrum.type": lambda: s.MDRamanSpectrum(list(a), DT),
        "MDRamanEnsemble.empty": lambda: s.MDRamanEnsemble([], DT),
        "MDRamanEnsemble.shape": lambda: s.MDRamanEnsemble([a, a[:, 0]], DT),
        "PartialMDRamanSpectrum.shape": lambda: s.PartialMDRamanSpectrum(a, DT),
        "PartialMDRamanEnsemble.empty": lambda: s.PartialMDRamanEnsemble([], DT),
        "PartialMDRamanEnsemble.groups_differ": lambda: s.PartialMDRamanEnsemble([g, g[:, :2]], DT),
        "ModeMDRamanSpectrum.shape": lambda: s.ModeMDRamanSpectrum(a, DT),
        "ModeMDRamanSpectrum.no_channel": lambda: s.ModeMDRamanSpectrum(c[:, :0], DT),
        "ModeMDRamanEnsemble.empty": lambda: s.ModeMDRamanEnsemble([], DT),
        "ModeMDRamanEnsemble.no_channel": lambda: s.ModeMDRamanEnsemble([c[:, :0]], DT),
        "ModeMDRamanEnsemble.channels_differ": lambda: s.ModeMDRamanEnsemble([c, c[:, :2]], DT),
        "ModeMDRamanSpectrum.two_frames": lambda: s.ModeMDRamanSpectrum(c[:1], DT).measure(),
        "ModeMDRamanEnsemble.two_frames": lambda: s.ModeMDRamanEnsemble([c[:1], c[:1]], DT).measure(),
        "VibrationalDensityOfStates.shape": lambda: s.VibrationalDensityOfStates(p[:, :, :2], DT, lattice),
        "VibrationalDensityOfStates.lattice_shape": lambda: s.VibrationalDensityOfStates(p, DT, data["lattices_r21"]),
        "VibrationalDensityOfStates.lattice_singular": lambda: s.VibrationalDensityOfStates(p, DT, np.zeros((3, 3))),
        "VibrationalDensityOfStates.masses": lambda: s.VibrationalDensityOfStates(p, DT, lattice, -masses),
        "VibrationalDensityOfStates.labels": lambda: s.VibrationalDensityOfStates(
            p, DT, lattice, masses, [0, 1, 2, 3, 4], 3),
        "VibrationalDensityOfStates.num_groups": lambda: s.VibrationalDensityOfStates(p, DT, lattice, masses, None, 2),
        "VibrationalDensityOfStatesEnsemble.empty": lambda: s.VibrationalDensityOfStatesEnsemble([], DT, lattice),
        "VibrationalDensityOfStatesEnsemble.atoms_differ": lambda: s.VibrationalDensityOfStatesEnsemble(
            [p, p[:, :4]], DT, lattice),
        "VibrationalDensityOfStatesEnsemble.lattices": lambda: s.VibrationalDensityOfStatesEnsemble(
            [p, p], DT, [data["lattices_s33"]]),
        "ModeVibrationalDensityOfStates.vectors_shape": lambda: s.ModeVibrationalDensityOfStates(
            p, DT, lattice, vectors[:, :4]),
        "ModeVibrationalDensityOfStates.too_many": lambda: s.ModeVibrationalDensityOfStates(
            p, DT, lattice, np.ones((16, 5, 3))),
        "ModeVibrationalDensityOfStatesEnsemble.empty": lambda: s.ModeVibrationalDensityOfStatesEnsemble(
            [], DT, lattice, vectors),
    }
    if gpu:
        import torch

        def t(array):
            return torch.tensor(np.ascontiguousarray(array), dtype=torch.float64, device="cuda:0")
        lengths = {"run_lengths": [20, 14]}
        cases.update({
            "DeviceMDRamanSpectrum.shape": lambda: s.DeviceMDRamanSpectrum(t(a[:, :2]), DT),
            "DeviceMDRamanSpectrum.strided": lambda: s.DeviceMDRamanSpectrum(t(a)[::2], DT),
            "DeviceMDRamanSpectrum.cpu": lambda: s.DeviceMDRamanSpectrum(torch.tensor(a), DT),
            "DeviceMDRamanSpectrum.float32": lambda: s.DeviceMDRamanSpectrum(t(a).float(), DT),
            "DeviceMDRamanEnsemble.empty": lambda: s.DeviceMDRamanEnsemble([], DT),
            "DeviceMDRamanEnsemble.no_lengths": lambda: s.DeviceMDRamanEnsemble(t(a), DT),
            "DeviceMDRamanEnsemble.lengths": lambda: s.DeviceMDRamanEnsemble(t(a), DT, **lengths),
            "DeviceMDRamanEnsemble.zero_length": lambda: s.DeviceMDRamanEnsemble(t(a), DT, run_lengths=[33, 0]),
            "DeviceMDRamanEnsemble.no_length": lambda: s.DeviceMDRamanEnsemble(t(a), DT, run_lengths=[]),
            "DeviceMDRamanEnsemble.lengths_with_sequence": lambda: s.DeviceMDRamanEnsemble([t(a)], DT, run_lengths=[33]),
            "DeviceMDRamanEnsemble.cpu": lambda: s.DeviceMDRamanEnsemble([torch.tensor(a)], DT),
            "DevicePartialMDRamanSpectrum.shape": lambda: s.DevicePartialMDRamanSpectrum(t(a), DT),
            "DevicePartialMDRamanSpectrum.strided": lambda: s.DevicePartialMDRamanSpectrum(t(g)[:, ::2], DT),
            "DevicePartialMDRamanEnsemble.empty": lambda: s.DevicePartialMDRamanEnsemble([], DT),
            "DevicePartialMDRamanEnsemble.lengths": lambda: s.DevicePartialMDRamanEnsemble(t(g), DT, run_lengths=[17, 16]),
            "DevicePartialMDRamanEnsemble.no_lengths": lambda: s.DevicePartialMDRamanEnsemble(t(g), DT),
            "DevicePartialMDRamanEnsemble.lengths_with_sequence": lambda: s.DevicePartialMDRamanEnsemble(
                [t(g)], DT, run_lengths=[33]),
            "DeviceModeMDRamanSpectrum.shape": lambda: s.DeviceModeMDRamanSpectrum(t(a), DT),
            "DeviceModeMDRamanSpectrum.no_channel": lambda: s.DeviceModeMDRamanSpectrum(t(c[:, :0]), DT),
            "DeviceModeMDRamanEnsemble.arrays": lambda: s.DeviceModeMDRamanEnsemble([c], DT),
            "DeviceModeMDRamanEnsemble.lengths": lambda: s.DeviceModeMDRamanEnsemble(t(c), DT, run_lengths=[17, 17]),
            "DeviceModeMDRamanEnsemble.no_channel": lambda: s.DeviceModeMDRamanEnsemble(
                t(c[:, :0]), DT, run_lengths=[17, 16]),
            "DeviceVibrationalDensityOfStates.shape": lambda: s.DeviceVibrationalDensityOfStates(
                t(p[:, :, :2]), DT, lattice),
            "DeviceVibrationalDensityOfStates.cpu": lambda: s.DeviceVibrationalDensityOfStates(torch.tensor(p), DT, lattice),
            "DeviceVibrationalDensityOfStates.lattice_strided": lambda: s.DeviceVibrationalDensityOfStates(
                t(p), DT, t(np.concatenate([data["lattices_s33"]] * 2))[::2]),
            "DeviceVibrationalDensityOfStates.lattice_shape": lambda: s.DeviceVibrationalDensityOfStates(
                t(p), DT, t(data["lattices_r21"])),
            "DeviceVibrationalDensityOfStatesEnsemble.lengths": lambda: s.DeviceVibrationalDensityOfStatesEnsemble(
                t(p), DT, lattice, **lengths),
            "DeviceVibrationalDensityOfStatesEnsemble.empty": lambda: s.DeviceVibrationalDensityOfStatesEnsemble(
                [], DT, lattice),
            "DeviceModeVibrationalDensityOfStates.vectors": lambda: s.DeviceModeVibrationalDensityOfStates(
                t(p), DT, lattice, vectors[:, :4]),
            "DeviceModeVibrationalDensityOfStatesEnsemble.lengths_with_sequence":
                lambda: s.DeviceModeVibrationalDensityOfStatesEnsemble([t(p)], DT, lattice, vectors, run_lengths=[33]),
        })
    for name, build in cases.items():
        record.call(f"refused.{name}", lambda: type(build()).__name__)


# ----------------------------------------------------------------------------- dump / compare / latency
def digest(arrays) -> str:
    sha = hashlib.sha256()
    for name in sorted(arrays):
        value = np.ascontiguousarray(arrays[name])
        sha.update(f"{name}|{value.dtype.str}|{value.shape}|".encode())
        sha.update(value.tobytes())
    return sha.hexdigest()


def dump(directory: str, spectrum) -> None:
    import torch
    os.makedirs(directory, exist_ok=True)
    gpu = torch.cuda.is_available()
    data = inputs()
    host = Record()
    exercise(host, spectrum, data, gpu, device_pass=False)
    refusals(host, spectrum, data, False)
    np.savez(os.path.join(directory, "host.npz"), **host.arrays)
    refused = {"host": host.refused}
    print(f"host   {len(host.arrays):5d} arrays, {len(host.refused):4d} refused  sha256 {digest(host.arrays)}")
    if gpu:
        device = Record()
        exercise(device, spectrum, data, True, device_pass=True)
        refusals(device, spectrum, data, True)
        np.savez(os.path.join(directory, "device.npz"), **device.arrays)
        refused["device"] = device.refused
        print(f"device {len(device.arrays):5d} arrays, {len(device.refused):4d} refused  sha256 {digest(device.arrays)}")
    with open(os.path.join(directory, "refused.json"), "w", encoding="utf-8") as handle:
        json.dump(refused, handle, indent=1)


def same_bytes(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def largest_difference(a, b) -> float:
    if a.shape != b.shape or a.dtype.kind not in "fiu" or b.dtype.kind not in "fiu":
        return float("inf")
    if a.size == 0:
        return 0.0
    difference = np.abs(a.astype(np.float64) - b.astype(np.float64))
    if np.isnan(difference).any():
        return 0.0 if same_bytes(a, b) else float("inf")
    return float(difference.max())


def load(directory: str, name: str):
    path = os.path.join(directory, name)
    if not os.path.exists(path):
        return None
    with np.load(path) as archive:
        return {key: archive[key] for key in archive.files}


def compare(directories) -> int:
    failures = 0
    first, *others = directories
    # host paths and refused calls: byte for byte across every dump given
    reference = load(first, "host.npz")
    for other in others:
        arrays = load(other, "host.npz")
        names = sorted(set(reference) | set(arrays))
        different = [name for name in names
                     if name not in reference or name not in arrays or not same_bytes(reference[name], arrays[name])]
        print(f"host   {first} vs {other}: {len(names) - len(different)} of {len(names)} arrays byte for byte")
        for name in different:
            print(f"  DIFFERS {name}")
        failures += len(different)
    with open(os.path.join(first, "refused.json"), encoding="utf-8") as handle:
        refused = json.load(handle)
    for other in others:
        with open(os.path.join(other, "refused.json"), encoding="utf-8") as handle:
            theirs = json.load(handle)
        for part in sorted(set(refused) & set(theirs)):
            equal = refused[part] == theirs[part]
            print(f"refused ({part}) {first} vs {other}: {len(refused[part])} / {len(theirs[part])} "
                  f"{'equal' if equal else 'DIFFERENT'}")
            if not equal:
                failures += 1
                ours = {tuple(item) for item in refused[part]}
                for item in sorted({tuple(item) for item in theirs[part]} ^ ours):
                    print(f"  {item}")
    # device paths
    device = [load(directory, "device.npz") for directory in directories]
    if any(arrays is None for arrays in device):
        print("device: not in every dump, not compared")
        return failures
    if len(device) == 2:
        a, b = device
        names = sorted(set(a) | set(b))
        different = [name for name in names if name not in a or name not in b or not same_bytes(a[name], b[name])]
        print(f"device {directories[0]} vs {directories[1]}: {len(names) - len(different)} of {len(names)} arrays "
              "byte for byte")
        for name in different:
            both = name in a and name in b
            print(f"  differs {name}: {largest_difference(a[name], b[name]) if both else 'missing'}")
        return failures
    a, b, c = device
    names = sorted(set(a) | set(b) | set(c))
    stable = [name for name in names if name in a and name in b and same_bytes(a[name], b[name])]
    unstable = [name for name in names if name not in stable]
    broken = [name for name in stable if name not in c or not same_bytes(a[name], c[name])]
    print(f"device: {len(names)} arrays; the parent's two dumps agree byte for byte on {len(stable)}; "
          f"the new tree agrees with them on {len(stable) - len(broken)}")
    for name in broken:
        print(f"  DIFFERS {name}: {largest_difference(a[name], c[name]) if name in c else 'missing'}")
    failures += len(broken)
    for name in unstable:
        if not (name in a and name in b and name in c):
            print(f"  MISSING {name}")
            failures += 1
            continue
        own = largest_difference(a[name], b[name])
        new = max(largest_difference(a[name], c[name]), largest_difference(b[name], c[name]))
        verdict = "within" if new <= own else "ABOVE"
        failures += new > own
        print(f"  parent differs from itself: {name}: parent {own:.3e}, new {new:.3e}  {verdict}")
    return failures


def latency(spectrum) -> None:
    import torch
    data = inputs()

    def tensor(array):
        return torch.tensor(np.ascontiguousarray(array), dtype=torch.float64, device="cuda:0")
    whole = spectrum.DeviceMDRamanSpectrum(tensor(data["alpha_s33"]), DT)
    ensemble = spectrum.DeviceMDRamanEnsemble([tensor(data["alpha_r33"]), tensor(data["alpha_r21"])], DT)
    modes = spectrum.DeviceModeMDRamanSpectrum(tensor(data["channels_s33"]), DT)
    calls = {"DeviceMDRamanSpectrum.measure": whole.measure,
             "DeviceMDRamanEnsemble.measure_segments": lambda: ensemble.measure_segments(W, HOP),
             "DeviceModeMDRamanSpectrum.measure_interference": lambda: modes.measure_interference(BANDS)}
    result = {}
    for name, call in calls.items():
        for _ in range(50):
            call()
        times = []
        for _ in range(500):
            start = time.perf_counter()
            call()
            times.append(1e6 * (time.perf_counter() - start))
        result[name] = round(float(np.median(times)), 2)
    print(json.dumps(result))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    parser.add_argument("--dump", metavar="DIR")
    parser.add_argument("--compare", nargs="+", metavar="DIR")
    parser.add_argument("--latency", action="store_true")
    args = parser.parse_args()
    if args.compare:
        if len(args.compare) not in (2, 3):
            parser.error("--compare takes two or three directories")
        failures = compare(args.compare)
        print("OK" if not failures else f"FAILED: {failures}")
        return 1 if failures else 0
    import torch  # noqa: F401  (before the HIP library: one HIP runtime per process, torch's)
    sys.path.insert(0, os.path.abspath(args.tree))
    import ramannoodle_amd.spectrum as spectrum
    print(f"ramannoodle_amd.spectrum from {os.path.dirname(os.path.abspath(spectrum.__file__))}")
    if args.dump:
        dump(args.dump, spectrum)
    if args.latency:
        latency(spectrum)
    return 0


if __name__ == "__main__":
    sys.exit(main())
