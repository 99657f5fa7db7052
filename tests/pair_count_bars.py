"""Bars of the pair-count tests (tests/test_pair_counts.py, tests/test_pair_counts_cpu.py), in one place: 5 x the largest error
measured on the MI355X, the project's rule (tests/parity_bars.py).  Metric everywhere: max over the entries of
|C - reference| / max(1, reference).
"""

# the loop-form float64 statement (tests/pair_count_oracle.loop_form) against the dense oracle on the GPU grid's inputs: the
# float64 rounding floor of the kernel's form
LOOP_FORM_FLOOR_BAR = 4.7e-14  # measured worst 9.44e-15 (K = 16)

# test_pair_counts_against_the_oracle: K = 4, 8, 12 padded, 16, 32, 64; both parameter layouts; W = 0 / 37; ragged lens; a serial
# and a segmented plan; rows of 700 sites.  The float64 figure sits at the loop form's floor above (9.4e-15).
F32_COUNTS_BAR = 4.9e-5  # measured worst 9.91e-6 (K = 32); K = 16, the matrix-instruction path: 4.50e-6
F64_COUNTS_BAR = 6.7e-14  # measured worst 1.35e-14 (K = 32)

# test_long_row_keeps_its_small_entries: K = 16 float32, one row of 40,000 sites at 1 % hets, float32 sums added into the float64
# partial every 64 sites (64 * 2^-24 = 3.8e-6, below F32_COUNTS_BAR)
F32_LONG_ROW_BAR = 2.6e-5  # measured 5.35e-6 (both plans)
# ... and its entries at least 8 states off the diagonal (2e-20 .. 8e-6), relative to the entry itself
F32_LONG_ROW_FAR_REL_BAR = 3.8e-5  # measured 7.80e-6 (both plans)

# identities against phk_transitions (bin = 1) and phk_posterior on the same handle, K = 16, rows of 5,000 sites, ragged lens,
# relative to max(1, reference)
F32_ARRIVALS_IDENTITY_BAR = 7.3e-7  # measured worst 1.48e-7 (segmented plan)
F64_ARRIVALS_IDENTITY_BAR = 2.9e-14  # measured worst 5.91e-15 (serial plan)
F32_MARGINALS_IDENTITY_BAR = 6.6e-7  # measured worst 1.33e-7 (segmented plan)
F64_MARGINALS_IDENTITY_BAR = 2.9e-14  # measured worst 5.81e-15 (serial plan)
# |counts.sum() - own scored sites| / own scored sites, over every test that states it
F32_TOTAL_BAR = 4.4e-7  # measured worst 8.94e-8 (the golden contig, 100 windows)
F64_TOTAL_BAR = 7.5e-15  # measured worst 1.52e-15
