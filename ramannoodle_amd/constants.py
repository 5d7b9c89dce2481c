"""Constants used on the evaluation path (``ramannoodle/constants.py:248-249``)."""

RAMAN_TENSOR_CENTRAL_DIFFERENCE = 0.001
BOLTZMANN_CONSTANT = 8.617333262e-5  # eV/K
REDUCED_PLANCK_CONSTANT = 0.6582119569  # eV fs (an addition: the quantum amplitudes of ramannoodle_amd/harmonic.py)
