"""HIP-event time of a local likelihood-ratio call (bin = 1 and bin = 100) against a tract-posterior call and a posterior-decoding
call (mean track) at the same bin on the same inputs, K = 16, float32 kernels (not run by bench.py).

Shapes: (b) 100 models x 20 rows x 100,000 windows; (c) the reference's production shape, 500 x 5 x 100,000; both at 5 % hets.
The alternative is every model's own block with theta doubled (a block per model).  Before it reports a shape the script checks
the log ratios against the float64 dense oracle of tests/local_oracle.py on two (model, row) pairs, and prints one JSON line per
shape and bin with the library's sha256.

    python scripts/local_ratio_timing.py [--shapes bc] [--bins 1,100] [--reps 5]
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

SHAPES = {"b": (100, 20, 100_000, 0.05), "c": (500, 5, 100_000, 0.05)}


def rows(S, L, het, seed):
    g = np.random.default_rng(seed)
    d = (g.random((S, L), dtype=np.float32) < het).astype(np.int8)
    d.flat[g.integers(0, d.size, size=int(0.01 * d.size))] = -1
    d[:, 0] = 1
    return d


def timed(fns, reps):
    """medians (ms) of ``reps`` alternating calls of every function after one warm-up call of each"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bc")
    ap.add_argument("--bins", default="1,100")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel
    from phlash_amd.synth import particle_population
    import local_bars as bars
    import local_oracle as lo
    from oracle import psmc_numpy as pn

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    m = (np.arange(16) < 11).astype(np.float64)  # the tract call's set: the eleven youngest states
    bins = tuple(int(b) for b in args.bins.split(","))
    for key in args.shapes:
        B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        dm = tmpl.from_flat(x).to_dm()
        pp = PSMCParams.from_dm(dm)
        pa = PSMCParams.from_dm(DemographicModel(eta=dm.eta, theta=dm.theta * 2.0, rho=dm.rho))
        P = pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64
        A = pa.stack()[:, None].cuda()
        f = torch.as_tensor(dm.eta.ect(), dtype=torch.float64).reshape(-1, 16).expand(B, 16).contiguous().cuda()
        w = torch.as_tensor(m).cuda()
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        pairs = ((0, 0), (B - 1, S - 1))
        np_of = lambda p, b: pn.PP(*(getattr(p, name)[b].numpy() for name in pn.PP._fields))  # noqa: E731
        refs = [lo.dense(np_of(pp, b), np_of(pa, b), data[s], 0, bins) for b, s in pairs]
        for g, bin in enumerate(bins):
            ll, lr = eng.local_ratio(P, A, inds, 0, bin=bin)
            assert not eng.underflow_risk()
            assert torch.isfinite(lr).all()
            ll0, _, _ = eng.posterior(P, inds, 0, values=f, bin=bin, marginals=False, mean=True)
            assert torch.equal(ll, ll0)
            worst = 0.0
            for (b, s), (ref, llr) in zip(pairs, refs):
                got = lr[b, s].double().cpu().numpy()
                worst = max(worst, float((np.abs(got - ref[g]) / np.maximum(1.0, np.abs(ref[g]))).max()))
                assert abs(float(ll[b, s]) / llr - 1) < 1e-5
            assert worst < bars.F32_LOCAL_BAR, worst
            check = (f"log ratio vs float64 oracle on 2 sequences: max |err| / max(1, |log ratio|) {worst:.1e} (mean log ratio "
                     f"{float(lr.double().mean()):.3f}); ll bitwise phk_posterior's")
            t_lr, t_tr, t_dec = timed([lambda: eng.local_ratio(P, A, inds, 0, bin=bin), lambda: eng.tracts(P, inds, w, 0, bin=bin),
                                       lambda: eng.posterior(P, inds, 0, values=f, bin=bin, marginals=False, mean=True)], args.reps)
            print(json.dumps({"shape": key, "B": B, "S": S, "L": L, "het": het, "bin": bin, "local_ratio_ms": round(t_lr, 3),
                              "tracts_ms": round(t_tr, 3), "posterior_ms": round(t_dec, 3), "ratio_to_tracts": round(t_lr / t_tr, 3),
                              "ratio_to_posterior": round(t_lr / t_dec, 3), "plan": eng.get_plan(), "check": check,
                              "lib_sha256": sha}), flush=True)
            del lr, ll
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
