"""HIP-event time of a posterior-decoding call (mean track, bin = 1) against a gradient call on the same inputs, K = 16,
float32 kernels (not run by bench.py).

Shapes: (a) one model x one 3,000,001-window row; (b) 100 models x 20 rows x 100,000 windows; (c) the reference's
production shape, 500 x 5 x 100,000 at 5 % hets.  Before it reports a shape the script checks the decode against the
float64 forward-backward of tests/posterior_oracle.py on a sample of (model, row) pairs ((a): its ll against the no-gradient
call and the identities, the oracle being a pure-Python loop), and prints one JSON line per shape with the library's
sha256.

    python scripts/decode_timing.py [--shapes abc] [--reps 5]
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

SHAPES = {"a": (1, 1, 3_000_001, 0.02), "b": (100, 20, 100_000, 0.02), "c": (500, 5, 100_000, 0.05)}
F32_GAMMA_BAR = 1.6e-5  # tests/test_posterior_decode.py


def rows(S, L, het, seed):
    g = np.random.default_rng(seed)
    d = (g.random((S, L), dtype=np.float32) < het).astype(np.int8)
    d.flat[g.integers(0, d.size, size=int(0.01 * d.size))] = -1
    d[:, 0] = 1
    return d


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population
    import posterior_oracle as po
    from oracle import psmc_numpy as pn

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    for key in args.shapes:
        B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        dm = tmpl.from_flat(x).to_dm()
        pp = PSMCParams.from_dm(dm)
        P = pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64
        f = torch.as_tensor(dm.eta.ect(), dtype=torch.float64).reshape(-1, 16).expand(B, 16).contiguous().cuda()
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        ll, mean, _ = eng.posterior(P, inds, 0, values=f, bin=1, marginals=False, mean=True)
        assert not eng.underflow_risk()
        assert torch.isfinite(mean).all()
        ll0 = eng.run(P, inds, 0, grad=False)
        llrel = float((ll / ll0 - 1).abs().max())
        assert llrel < 1e-6, llrel
        if key == "a":
            _, _, marg = eng.posterior(P, inds, 0, bin=1, marginals=True)
            mass = float((marg.double().sum(-1) - 1).abs().max())
            assert mass < 3e-5, mass
            check = f"ll rel to the no-gradient call {llrel:.1e}, |sum gamma - 1| {mass:.1e}"
            del marg
        else:
            worst = 0.0
            for b, s in ((0, 0), (B - 1, S - 1)):
                q = pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))
                g, llr = po.forward_backward(q, data[s], 0)
                ref = g @ f[b].cpu().numpy()
                worst = max(worst, float(np.abs(mean[b, s].double().cpu().numpy() - ref).max() / np.abs(ref).max()))
                assert abs(float(ll[b, s]) / llr - 1) < 1e-5
            assert worst < F32_GAMMA_BAR, worst
            check = f"mean track vs float64 oracle on 2 sequences: max rel {worst:.1e}; ll rel to the no-gradient call {llrel:.1e}"
        t_dec = timed(lambda: eng.posterior(P, inds, 0, values=f, bin=1, marginals=False, mean=True), args.reps)
        t_grad = timed(lambda: eng.run(P, inds, 0, grad=True), args.reps)
        plan = eng.get_plan()
        print(json.dumps({"shape": key, "B": B, "S": S, "L": L, "het": het, "decode_ms": round(t_dec, 3), "grad_ms": round(t_grad, 3),
                          "ratio": round(t_dec / t_grad, 3), "grad_plan": plan, "check": check, "lib_sha256": sha}), flush=True)
        del eng, mean, ll
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
