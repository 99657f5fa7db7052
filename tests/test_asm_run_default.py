"""The hand-written block-run sequence of the K = 16 float32 sweeps (csrc/sweep_run_k16r2.inc, scripts/gen_sweep_asm.py) is what a
new handle runs.  It performs the C++ body's arithmetic operation for operation -- an all-hom block without the per-site tests and
with the beta pass's suf(v.*w) kept for the forward pass, a mixed block with the tests -- so switching it off on the same handle
(``phk_set_asm_run(h, 0)``) must give the SAME BITS: log-likelihoods and every gradient row.

Shapes: the smallest that reach every path of the sequence.  33 particles x 2 chunks is a full two-row wave (32 sequences of two
lanes) plus a wave with one active group pair; 8 * 70 + 3 sites end in a partial block (general body) after runs of hot blocks; a
warm-up of 37 sites puts the boundary inside a block, which splits the runs; 2,600 sites make the fold of the partial sums into
float64 (every 2,048 sites) split a run.  Rows: no hets at all, 2 % and 30 % hets, each with 1 % missing sites and a run of 40
missing sites (all-hom blocks, mixed blocks with het lanes, mixed blocks with missing lanes)."""

import numpy as np
import pytest

from oracle import psmc_numpy as o

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _engine(K, data, dbl=False):
    from phlash_amd.engine import HipEngine

    return HipEngine(K, data, double_precision=dbl)


_PARAMS = {}


def _params(B, S):
    """B particles around the default model, K = 16 -> [B, S, 7, 16] (computed once per shape)"""
    if (B, S) not in _PARAMS:
        rng = np.random.default_rng(100 * B + S)
        pat = "14*1+1*2"
        x0 = o.particle_from_linear(pat, 1e-4, 15.0, np.ones(len(o.parse_pattern(pat))), 1e-2, 1e-2)
        out = np.zeros((B, S, 7, 16))
        for b in range(B):
            x = x0 + 0.3 * rng.normal(size=x0.shape) * (b > 0)
            out[b, :] = o.from_dm(o.particle_to_dm(x, pat, 1e-2)).stack()
        out.setflags(write=False)
        _PARAMS[(B, S)] = out
    return _PARAMS[(B, S)]


def _rows(S, L, het):
    rng = np.random.default_rng(int(1000 * het) + 7 * S + L)
    data = (rng.uniform(size=(S, L)) < het).astype(np.int8)
    data.flat[rng.integers(0, data.size, data.size // 100)] = -1
    data[0, L // 3:L // 3 + 40] = -1
    data[:, 0] = np.maximum(data[:, 0], 0)
    return data


def _run(eng, P, S, W):
    p = torch.tensor(P, device="cuda")
    i = torch.arange(S, dtype=torch.int64, device="cuda")
    ll, g = eng.run(p, i, warmup=W, grad=True)
    torch.cuda.synchronize()
    return ll.cpu().numpy(), g.double().cpu().numpy()


def _set_plan(eng, plan, B, S):
    eng.set_autotune(False)
    eng.set_rescale_interval(4)
    if plan == "serial":
        eng.set_plan(0, R=2, T=8, R_forward=1, R_scan=0)
    elif plan == "segmented":
        eng.set_plan(1, R=2, T=8, R_forward=16, R_scan=16)
    else:  # serial sweep of the first chunk's sequences beside the segment sweep of the rest
        eng.install_plan({"segmented": 0, "R": 2, "T": 8, "R_forward": 1, "hybrid_first": B * (S // 2), "R_segment_sweep": 2, "R_scan": 16})


def _on_equals_off(eng, P, S, W):
    assert eng.get_asm_run()  # nothing has switched it off
    ll_a, g_a = _run(eng, P, S, W)
    eng.set_asm_run(False)
    assert not eng.get_asm_run()
    ll_c, g_c = _run(eng, P, S, W)
    eng.set_asm_run(True)
    assert eng.get_asm_run()
    ll_b, g_b = _run(eng, P, S, W)
    assert np.isfinite(ll_c).all() and np.isfinite(g_c).all() and np.abs(g_c).max() > 0
    assert np.array_equal(ll_a, ll_c) and np.array_equal(ll_b, ll_c)
    assert np.array_equal(g_a, g_c), float(np.abs(g_a - g_c).max())
    assert np.array_equal(g_b, g_c), float(np.abs(g_b - g_c).max())


@pytest.mark.parametrize("het", [0.0, 0.02, 0.30])
@pytest.mark.parametrize("plan", ["serial", "segmented", "hybrid"])
def test_sequence_equals_the_cxx_body(plan, het):
    B, S, L, W = 33, 2, 8 * 70 + 3, 37
    eng = _engine(16, _rows(S, L, het))
    _set_plan(eng, plan, B, S)
    _on_equals_off(eng, _params(B, S), S, W)
    if plan == "hybrid":
        assert eng.get_plan().get("hybrid_first") == B
    else:
        assert eng.get_plan()["segmented"] == (plan == "segmented")


@pytest.mark.parametrize("plan", ["serial", "segmented"])
def test_a_float64_fold_splits_a_run(plan):
    """More than 2,048 sites: the run of hot blocks ends where the partial sums are folded, and the next one starts there."""
    B, S, L, W = 33, 1, 2600, 37
    eng = _engine(16, _rows(S, L, 0.02))
    _set_plan(eng, plan, B, S)
    _on_equals_off(eng, _params(B, S), S, W)


@pytest.mark.parametrize("plan", ["serial", "hybrid"])
def test_waves_of_more_than_two_rows_keep_the_cxx_loop(plan):
    """5 particles x 8 chunks: a wave of 32 sequences holds seven observation rows, the sequence's two-row masks do not apply,
    and the kernel takes the C++ loop whatever the handle asks for."""
    B, S, L, W = 5, 8, 8 * 70 + 3, 37
    eng = _engine(16, _rows(S, L, 0.02))
    _set_plan(eng, plan, B, S)
    _on_equals_off(eng, _params(B, S), S, W)


def test_default_of_a_new_handle(monkeypatch):
    """On for K = 16 float32, off -- there is no such sequence -- for K = 32, K = 64 and float64; PHK_ASM_RUN=0 in the environment
    selects the C++ body."""
    monkeypatch.delenv("PHK_ASM_RUN", raising=False)
    data = _rows(2, 64, 0.02)
    assert _engine(16, data).get_asm_run()
    for K, dbl in ((32, False), (64, False), (16, True), (32, True)):
        eng = _engine(K, data, dbl)
        assert not eng.get_asm_run(), (K, dbl)
        eng.set_asm_run(True)  # accepted, and without effect
        assert not eng.get_asm_run(), (K, dbl)
    monkeypatch.setenv("PHK_ASM_RUN", "0")
    eng = _engine(16, data)
    assert not eng.get_asm_run()
    eng.set_asm_run(True)
    assert eng.get_asm_run()
