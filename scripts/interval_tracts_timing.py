"""HIP-event time of an interval-tract call against tract-posterior calls on the same inputs, K = 16, float32 kernels (not run by
bench.py): phk_tracts at bin = 1 and bin = 100 (the yardstick: calls this sweep leaves untouched), phk_interval_tracts with (a)
intervals equal to the bins of 100 and (b) the Viterbi segments of the same rows under the first model, each with the states
within 1 of the segment's own as its set.

Shapes: (b) 100 models x 20 rows x 100,000 windows; (c) the reference's production shape, 500 x 5 x 100,000; both at 5 % hets.
Before it reports a shape the script checks the first intervals of two (model, row) pairs against the float64 oracle of
tests/interval_oracle.py, and (a) against the log of phk_tracts; it prints one JSON line per shape with the library's sha256.

    python scripts/interval_tracts_timing.py [--shapes bc] [--reps 5]
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from local_ratio_timing import SHAPES, rows, timed  # noqa: E402  (the same rows and the same clock)

N_CHECK = 40  # intervals per checked sequence


def csr(row, S):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(np.bincount(row, minlength=S))]), dtype=torch.int64, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bc")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.decode import tmrca_segments
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population
    import interval_bars as bars
    import interval_oracle as io
    from oracle import psmc_numpy as pn

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    m = (np.arange(16) < 11).astype(np.float64)  # the set of the tract calls and of (a): the eleven youngest states
    word = int(sum(1 << k for k in range(11)))
    for key in args.shapes:
        B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        pp = PSMCParams.from_dm(tmpl.from_flat(x).to_dm())
        P = pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64
        w = torch.as_tensor(m).cuda()
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int64, device="cuda")  # noqa: E731
        # (a) the bins of 100
        nb = L // 100
        row_a = np.repeat(np.arange(S), nb)
        start_a = np.tile(np.arange(nb) * 100, S)
        A = (csr(row_a, S), dev(start_a), dev(start_a + 100), dev(np.full(row_a.size, word)))
        # (b) the Viterbi segments of the rows under the first model (sorted by row and start as they come)
        _, path = eng.viterbi(P[:1], inds, 0)
        r, s0, e0, st = (t.cpu().numpy() for t in tmrca_segments(path[0]))
        near = np.array([sum(1 << k for k in range(max(z - 1, 0), min(z + 2, 16))) for z in st], dtype=np.int64)
        Bv = (csr(r, S), dev(s0), dev(e0), dev(near))
        max_b = int((e0 - s0).max())
        call_a = lambda: eng.interval_tracts(P, inds, *A, warmup=0, max_len=100)  # noqa: E731
        call_b = lambda: eng.interval_tracts(P, inds, *Bv, warmup=0, max_len=max_b)  # noqa: E731
        ll_a, lp_a = call_a()
        ll_b, lp_b = call_b()
        assert not eng.underflow_risk()
        ll_t, tr = eng.tracts(P, inds, w, 0, bin=100)
        assert torch.equal(ll_a, ll_t) and torch.equal(ll_b, ll_t)
        # (a) against the log of phk_tracts (an absolute error of p is bar / p as an error of its log), both against the oracle
        ref = torch.log(tr.double()).reshape(B, S * nb)
        fin = torch.isfinite(ref) & (ref > -20)
        vs_tracts = float((lp_a - ref)[fin].abs().max())
        np_of = lambda b: pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))  # noqa: E731
        worst = 0.0
        for b, s in ((0, 0), (B - 1, S - 1)):
            ja = np.flatnonzero(row_a == s)[:N_CHECK]
            jb = np.flatnonzero(r == s)[:N_CHECK]
            oa, llo = io.dense(np_of(b), data[s], 0, [(start_a[j], start_a[j] + 100, word) for j in ja])
            ob, _ = io.dense(np_of(b), data[s], 0, [(s0[j], e0[j], int(near[j])) for j in jb])
            for got, want in ((lp_a[b, ja].cpu().numpy(), oa), (lp_b[b, jb].cpu().numpy(), ob)):
                worst = max(worst, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
            assert abs(float(ll_a[b, s]) / llo - 1) < 1e-5
        assert worst < bars.F32_GRID_BAR, worst
        check = (f"first {N_CHECK} intervals of 2 sequences vs float64 oracle: max |err| / max(1, |logp|) {worst:.1e}; (a) vs log(phk_tracts) "
                 f"where logp > -20: max |diff| {vs_tracts:.1e}; ll bitwise phk_tracts'")
        t1, t100, ta, tb = timed([lambda: eng.tracts(P, inds, w, 0, bin=1), lambda: eng.tracts(P, inds, w, 0, bin=100), call_a, call_b], args.reps)
        print(json.dumps({"shape": key, "B": B, "S": S, "L": L, "het": het, "tracts_bin1_ms": round(t1, 3), "tracts_bin100_ms": round(t100, 3),
                          "interval_bins100_ms": round(ta, 3), "interval_viterbi_ms": round(tb, 3), "n_bins100": int(row_a.size),
                          "n_viterbi": int(r.size), "longest_viterbi": max_b, "a_over_tracts_bin100": round(ta / t100, 3),
                          "a_over_tracts_bin1": round(ta / t1, 3), "b_over_tracts_bin100": round(tb / t100, 3),
                          "b_over_tracts_bin1": round(tb / t1, 3), "plan": eng.get_plan(), "check": check, "lib_sha256": sha}), flush=True)
        del eng, lp_a, lp_b, tr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
