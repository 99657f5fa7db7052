"""HIP-event time of a Viterbi call (phk_viterbi) against a posterior-decoding call (phk_posterior, mean track, bin = 1) on
the same inputs, K = 16, float32 kernels (not run by bench.py).

Shapes (those of scripts/decode_timing.py): (a) one model x one 3,000,001-window row; (b) 100 models x 20 rows x 100,000
windows; (c) the reference's production shape, 500 x 5 x 100,000 at 5 % hets.  The two calls alternate in one process,
after a warm-up call of each; the medians of ``--reps`` calls are reported.  Before it reports a shape the script checks
the Viterbi call against the float64 oracle of tests/viterbi_oracle.py on a sample of (model, row) pairs: the path it
returns is valid, its float64 score is the kernel's logp, and what it gives up against the oracle's optimum stays under
the bar of tests/test_viterbi.py.  One JSON line per shape with the library's sha256.

    python scripts/viterbi_timing.py [--shapes abc] [--reps 5]
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


def rows(S, L, het, seed):
    g = np.random.default_rng(seed)
    d = (g.random((S, L), dtype=np.float32) < het).astype(np.int8)
    d.flat[g.integers(0, d.size, size=int(0.01 * d.size))] = -1
    d[:, 0] = 1
    return d


def timed_pair(f, g, reps):
    """medians (ms) of ``reps`` alternating calls of f and g after one warm-up call of each"""
    f()
    g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        for fn, ts in ((f, tf), (g, tg)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    return float(np.median(tf)), float(np.median(tg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population
    import test_viterbi as tv
    import viterbi_oracle as vo
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
        logp, path = eng.viterbi(P, inds, 0)
        assert not eng.underflow_risk()
        assert torch.isfinite(logp).all() and int(path.max()) < 16
        worst_def, worst_lp, ndiff, nsite = 0.0, 0.0, 0, 0
        for b, s in ((0, 0), (B - 1, S - 1)) if B * S > 1 else ((0, 0),):
            q = pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))
            z = path[b, s].cpu().numpy()
            assert tv._valid_path(q, z)
            own = vo.path_logp(q, data[s], z, 0)
            ref, best, _ = vo.viterbi(q, data[s], 0, want_margin=False)
            assert best - own >= -1e-9 * abs(best), best - own
            deficit = vo.deficit(q, data[s], ref, z, 0)  # term by term
            worst_def = max(worst_def, deficit / L)
            worst_lp = max(worst_lp, abs(float(logp[b, s]) / own - 1))
            ndiff += int((z != ref).sum())
            nsite += L
        assert worst_lp < tv.F32_LOGP_BAR, worst_lp
        assert worst_def <= tv.F32_VITERBI_DEFICIT_BAR, worst_def
        check = (f"{nsite // L} sequence(s) vs the float64 oracle: deficit per site {worst_def:.1e}, logp rel to the float64 score of "
                 f"the path {worst_lp:.1e}, {ndiff} of {nsite} sites differ from the oracle's path")
        t_vit, t_dec = timed_pair(lambda: eng.viterbi(P, inds, 0),
                                  lambda: eng.posterior(P, inds, 0, values=f, bin=1, marginals=False, mean=True), args.reps)
        print(json.dumps({"shape": key, "B": B, "S": S, "L": L, "het": het, "viterbi_ms": round(t_vit, 3), "posterior_ms": round(t_dec, 3),
                          "ratio": round(t_vit / t_dec, 3), "check": check, "lib_sha256": sha}), flush=True)
        del eng, path, logp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
