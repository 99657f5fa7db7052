"""Bars of the transition-posterior tests (tests/test_transitions.py), in one place: 5 x the largest error measured on the
MI355X over the grid of test_transitions_against_the_oracle (K = 4, 8, 12 padded, 16, 32, 64; both parameter layouts; W = 0 / 37;
bins 1 / 7 / 100; ragged lens), the project's rule (tests/parity_bars.py).

``arrivals``: largest absolute error of the bin means of (stay, up, down) against the float64 dense oracle.
``changes``: largest error of the bin sums of (sum_k up, sum_k down) relative to max(1, oracle).
"""

F32_ARRIVALS_BAR = 1.8e-5  # measured worst 3.63e-6 (K = 8)
F64_ARRIVALS_BAR = 3.0e-14  # measured worst 6.00e-15 (K = 8)
F32_CHANGES_BAR = 1.0e-5  # measured worst 2.07e-6 (K = 8)
F64_CHANGES_BAR = 2.1e-14  # measured worst 4.11e-15 (K = 8)

# L * arrivals at W = 0, bin = L against the gradient call's theta * d ll / d theta rows (d, v, b), float64, relative to the
# row kind's largest entry: 5 x the measured 4.68e-15 (d row; v 2.57e-15, b 3.39e-15)
F64_GRADIENT_IDENTITY_BAR = 2.3e-14

# the structured float64 statement (tests/transition_oracle.structured) against the dense oracle on the GPU grid's inputs:
# the float64 rounding floor of the kernel's form
STRUCTURED_FLOOR_BAR = 3.7e-14  # measured worst 7.44e-15 (K = 16)
