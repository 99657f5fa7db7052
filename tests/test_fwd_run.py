"""The hand-written run of lean pieces of the K = 16 float32 checkpointing forward kernel (csrc/fwd_run_k16r1.inc,
scripts/gen_fwd_asm.py; ``phk_set_fwd_run``).  It performs Lane::fwd_site<false> operation for operation -- an all-hom block without
the per-site tests, a mixed block with them, rescale on demand behind one compare per rescale site, the checkpoint stores from a
wave-uniform base -- so switching it off on the same handle must give the SAME BYTES: log-likelihoods, every
gradient row (the sweeps read the checkpoints and block exponents the kernel wrote), the per-sequence counts of rescaled blocks,
and the flag word.

Shapes: the smallest that reach every path of the run.  70 particles x 3 chunks are 210 sequences, stored chunk-major: waves that
hold one observation row, waves that hold two, and a partial last wave.  64 * 11 + 29 sites are eleven lean pieces and a ragged
tail; a warm-up of 37 sites puts the boundary inside the first piece, which then takes the C++ body and the run starts behind it.
Rows: het rates 0, 1 %, 10 %, 30 %, each with 1 % isolated missing sites and a run of 120 missing sites in row 0; row 1 begins and
ends with all-hom blocks."""

import os
import sys

import numpy as np
import pytest

from oracle import psmc_numpy as o

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, L = 70, 3, 64 * 11 + 29


def _engine(K, data, dbl=False):
    from phlash_amd.engine import HipEngine

    return HipEngine(K, data, double_precision=dbl)


_PARAMS = {}


def _params(nb):
    """nb particles around the default model, K = 16 -> [nb, 1, 7, 16] (computed once per size)"""
    if nb not in _PARAMS:
        rng = np.random.default_rng(500 + nb)
        pat = "14*1+1*2"
        x0 = o.particle_from_linear(pat, 1e-4, 15.0, np.ones(len(o.parse_pattern(pat))), 1e-2, 1e-2)
        out = np.zeros((nb, 1, 7, 16))
        for b in range(nb):
            x = x0 + 0.3 * rng.normal(size=x0.shape) * (b > 0)
            out[b, 0] = o.from_dm(o.particle_to_dm(x, pat, 1e-2)).stack()
        out.setflags(write=False)
        _PARAMS[nb] = out
    return _PARAMS[nb]


def _rows(ns, het):
    rng = np.random.default_rng(int(1000 * het) + 7 * ns + L)
    data = (rng.uniform(size=(ns, L)) < het).astype(np.int8)
    data.flat[rng.integers(0, data.size, data.size // 100)] = -1
    data[0, 200:320] = -1            # a run of 120 missing sites: whole blocks, and two pieces, of nothing else
    if ns > 1:                       # a row whose first block, last lean block and last full blocks are hom throughout
        data[1, :8] = 0
        data[1, 64 * 11 - 8:64 * 11 + 24] = 0
    data[:, 0] = np.maximum(data[:, 0], 0)
    return data


def _set_plan(eng, plan, nb, ns):
    """every plan with the forward kernel of one lane per sequence, 8 sites per block, rescale interval 4: the kernel that has the run"""
    eng.set_autotune(False)
    eng.set_rescale_interval(4)
    if plan == "serial":
        eng.set_plan(0, R=2, T=8, R_forward=1, R_scan=0)
    elif plan == "segmented":
        eng.set_plan(1, R=2, T=8, R_forward=1, R_scan=16)
    else:  # serial sweep of the first chunk's sequences beside the segment sweep of the rest
        eng.install_plan({"segmented": 0, "R": 2, "T": 8, "R_forward": 1, "hybrid_first": nb * max(ns // 2, 1), "R_segment_sweep": 2, "R_scan": 16})


def _outputs(eng, P, ns, W, grad=True):
    """everything a call hands back, as raw bytes"""
    p = torch.tensor(P, device="cuda")
    i = torch.arange(ns, dtype=torch.int64, device="cuda")
    res = eng.run(p, i, warmup=W, grad=grad)
    torch.cuda.synchronize()
    if not grad:
        out = {"ll": res.cpu().numpy().tobytes()}
    else:
        counts, blocks = eng.block_rescale_counts()
        out = {"ll": res[0].cpu().numpy().tobytes(), "grad": res[1].cpu().numpy().tobytes(), "rescaled blocks": counts.tobytes() + bytes([blocks % 256])}
        assert np.isfinite(res[1].cpu().numpy()).all()
    out["flag"] = eng.underflow_risk()
    return out


def _on_equals_off(eng, P, ns, W, grad=True):
    assert eng.get_fwd_run()
    on = _outputs(eng, P, ns, W, grad)
    eng.set_fwd_run(False)
    assert not eng.get_fwd_run()
    off = _outputs(eng, P, ns, W, grad)
    eng.set_fwd_run(True)
    again = _outputs(eng, P, ns, W, grad)
    for k in off:
        assert on[k] == off[k], k
        assert again[k] == off[k], k
    assert not off["flag"]
    return off


@pytest.mark.gpu
@pytest.mark.parametrize("W", [0, 37])
@pytest.mark.parametrize("het", [0.0, 0.01, 0.10, 0.30])
@pytest.mark.parametrize("plan", ["serial", "hybrid", "segmented"])
def test_run_equals_the_cxx_body(plan, het, W):
    eng = _engine(16, _rows(S, het))
    _set_plan(eng, plan, B, S)
    eng.set_fwd_run(True)
    _on_equals_off(eng, _params(B), S, W)
    assert eng.get_plan()["R_forward"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("W", [0, 37])
@pytest.mark.parametrize("plan", ["serial", "hybrid", "segmented"])
def test_without_a_gradient(plan, W):
    """no checkpoints: that kernel keeps the C++ body whatever the switch says, under every plan"""
    eng = _engine(16, _rows(S, 0.01))
    _set_plan(eng, plan, B, S)
    eng.set_fwd_run(True)
    _on_equals_off(eng, _params(B), S, W, grad=False)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["serial", "hybrid"])
def test_rescale_fires_inside_the_run(plan):
    """Particles steep enough for the on-demand rescale to fire inside blocks: the model and the het runs of
    tests/test_hip_parity.py::test_steep_blocks_take_the_general_body (emis1 = 1e-3, runs of 8 ... 24 het sites)."""
    from test_hip_parity import _params as parity_params

    P = np.repeat(parity_params(16, 2, 1, seed=3), B // 2, axis=0)
    P[:, 0, 5] = 1e-3
    P[:, 0, 4] = 1.0 - 1e-3
    rng = np.random.default_rng(7)
    data = (rng.uniform(size=(S, L)) < 0.01).astype(np.int8)
    for r in range(S):
        for s0, n in ((40 + 7 * r, 8), (301, 16), (640 + r, 24), (700, 9)):
            data[r, s0:s0 + n] = 1
    eng = _engine(16, data)
    _set_plan(eng, plan, B, S)
    eng.set_fwd_run(True)
    for W in (0, 37):
        _on_equals_off(eng, P, S, W)
        counts, blocks = eng.block_rescale_counts()
        # (eight hets of emis1 / emis0 = 1e-3 take 2^-80, the trigger is 2^-16: every sequence is rescaled inside its het runs)
        assert blocks == (L + 7) // 8 and counts.min() >= 1, (counts.min(), blocks)


@pytest.mark.gpu
def test_rows_shorter_than_the_matrix():
    """own lengths per row (the sweeps' ``lens``): rows end inside a lean piece, at a piece boundary and at the matrix's end"""
    data = _rows(S, 0.01)
    eng = _engine(16, data)
    _set_plan(eng, "serial", B, S)
    eng.set_fwd_run(True)
    p = torch.tensor(_params(B), device="cuda")
    i = torch.arange(S, dtype=torch.int64, device="cuda")
    lens = torch.tensor([64 * 5 + 13, 64 * 7, L], dtype=torch.int64, device="cuda")
    got = {}
    for on in (True, False):
        eng.set_fwd_run(on)
        ll, counts = eng.pair_counts(p, i, warmup=0, lens=lens)
        torch.cuda.synchronize()
        got[on] = (ll.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes())
        assert not eng.underflow_risk()
    assert got[True] == got[False]


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["serial", "hybrid"])
def test_waves_of_more_than_two_rows_keep_the_cxx_loop(plan):
    """20 particles x 4 chunks: the first wave holds four observation rows, the run's two-row code words do not apply, and the
    kernel takes the C++ loop whatever the handle asks for.  Same outputs, clean flag word."""
    nb, ns = 20, 4
    eng = _engine(16, _rows(ns, 0.10))
    _set_plan(eng, plan, nb, ns)
    eng.set_fwd_run(True)
    out = _on_equals_off(eng, _params(nb), ns, 37)
    assert not out["flag"]


@pytest.mark.gpu
def test_loop_budget_is_honoured_inside_the_run():
    """A budget of a few pieces runs out inside the run of lean pieces: the kernel returns, the flag query names kernel, sequence
    and block, and they are the same with the run on and off.  One wave (40 sequences of one row): one reporter."""
    from phlash_amd import _lib

    nb = 40
    eng = _engine(16, _rows(1, 0.01))
    _set_plan(eng, "serial", nb, 1)
    eng.set_fwd_run(True)
    ok = _outputs(eng, _params(nb), 1, 0)
    msgs = {}
    for on in (True, False):
        eng.set_fwd_run(on)
        eng.set_loop_budget_scale(1, 1, 32)  # 2 * 92 / 32 = 5 outer iterations for 11 lean pieces
        p = torch.tensor(_params(nb), device="cuda")
        eng.run(p, torch.arange(1, dtype=torch.int64, device="cuda"), warmup=0, grad=True)
        torch.cuda.synchronize()
        with pytest.raises(_lib.KernelOverrun, match="fwd_kernel") as e:
            eng.underflow_risk()
        msgs[on] = str(e.value)
        assert not eng.underflow_risk()  # reported once, then clear
        eng.set_loop_budget_scale(7, 1, 1)
    assert msgs[True] == msgs[False], msgs
    eng.set_fwd_run(True)
    assert _outputs(eng, _params(nb), 1, 0) == ok  # back to the real budget: the same bytes as before


@pytest.mark.gpu
def test_switch_of_a_new_handle(monkeypatch):
    """The switch exists for K = 16 float32 handles and is 0 -- there is no such sequence -- for K = 32, K = 64 and float64 whatever
    is asked; PHK_FWD_RUN in the environment decides what a new handle starts with; the plan a handle reports does not depend on it."""
    from phlash_amd import _lib

    monkeypatch.delenv("PHK_FWD_RUN", raising=False)
    data = _rows(2, 0.01)
    eng = _engine(16, data)
    assert eng.get_fwd_run() and _lib.load().phk_get_fwd_run(eng._h) == 1  # on for a new K = 16 float32 handle
    plan = eng.get_plan()
    eng.set_fwd_run(True)
    assert eng.get_fwd_run()
    eng.set_fwd_run(False)
    assert not eng.get_fwd_run() and eng.get_plan() == plan
    for K, dbl in ((32, False), (64, False), (16, True), (32, True)):
        e = _engine(K, data, dbl)
        assert not e.get_fwd_run(), (K, dbl)
        e.set_fwd_run(True)  # accepted, and without effect
        assert not e.get_fwd_run(), (K, dbl)
    monkeypatch.setenv("PHK_FWD_RUN", "0")
    eng = _engine(16, data)
    assert not eng.get_fwd_run()
    eng.set_fwd_run(True)
    assert eng.get_fwd_run()
    monkeypatch.setenv("PHK_FWD_RUN", "1")
    assert _engine(16, data).get_fwd_run()
    assert not _engine(32, data).get_fwd_run()


@pytest.mark.gpu
def test_a_library_built_without_the_run_refuses_it(tmp_path):
    """-DPHK_FWD_RUN=0: phk_api.hip compiled with the macro into a side library (its launchers and kernels are the shipped
    library's, which it links against) answers on = 1 with PHK_EUNSUPPORTED, on = 0 with PHK_OK, and reports the switch as 0.
    (The forward object is not built a second time here -- a minute of compiling; built with the macro its device code is the
    parent commit's byte for byte, profiles/ab_fwd_run.txt item 2.)"""
    import ctypes
    import subprocess

    from phlash_amd import _lib

    csrc = os.path.join(ROOT, "phlash_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj, side = str(tmp_path / "phk_api_norun.o"), str(tmp_path / "libphk_norun.so")
    flags = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17"]
    subprocess.run([hipcc, *flags, "-DPHK_FWD_RUN=0", "-c", os.path.join(csrc, "phk_api.hip"), "-o", obj], check=True, capture_output=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", side, obj, _lib.LIB_PATH,
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], check=True, capture_output=True)
    lib = ctypes.CDLL(side)
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.phk_create.argtypes, lib.phk_create.restype = [ctypes.POINTER(vp), i, vp, i64, i64, i, i, i], i
    for name, args in (("phk_set_fwd_run", [vp, i]), ("phk_get_fwd_run", [vp]), ("phk_set_asm_run", [vp, i]), ("phk_destroy", [vp])):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, i
    data = np.ascontiguousarray(_rows(2, 0.01))
    h = vp()
    assert lib.phk_create(ctypes.byref(h), 16, data.ctypes.data, data.shape[0], data.shape[1], 0, 0, 0) == _lib.PHK_OK
    try:
        assert lib.phk_get_fwd_run(h) == 0  # a K = 16 float32 handle of such a library starts without it
        assert lib.phk_set_fwd_run(h, 1) == _lib.PHK_EUNSUPPORTED
        assert lib.phk_get_fwd_run(h) == 0
        assert lib.phk_set_fwd_run(h, 0) == _lib.PHK_OK
        assert lib.phk_get_fwd_run(h) == 0
        assert lib.phk_set_asm_run(h, 1) == _lib.PHK_OK  # (the sweeps' switch is another macro's)
    finally:
        lib.phk_destroy(h)


# ---- static counts: CPU, from the generator and the build -------------------------------------------------------------------

PARENT_TRIP = 496   # instructions of the C++ body's trip through the block loop (the compiler's one body, tests included)
ALL_HOM_TARGET = 460


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_fwd_asm

    return gen_fwd_asm


@pytest.mark.parametrize("stores", ["spread", "clustered"])
def test_trip_counts(stores):
    """One trip through the block loop: the all-hom body holds the arithmetic -- 8 x (15 fma + 15 add + 24 packed) and the two
    sums of the rescale sites -- two compares, no v_mov, five stores, and no wait state."""
    g = _generator()
    lines, nops, top = g.build(stores)
    c = g.trip_counts(lines)
    hom, mixed = c["all-hom"], c["mixed"]
    assert nops == 0 and hom["s_nop"] == 0 and mixed["s_nop"] == 0
    assert hom["total"] <= ALL_HOM_TARGET < PARENT_TRIP and mixed["total"] < PARENT_TRIP, (hom, mixed)
    assert hom["packed"] == 192 and hom["v_fma"] == 120 and hom["v_add"] == 122 and hom["v_mov"] == 0 and hom["stores"] == 5 and hom["loads"] == 0
    assert mixed["v_mov"] == 0 and mixed["packed"] == 192 and mixed["branch"] == hom["branch"] + 9 and mixed["stores"] == 5 and mixed["loads"] == 0
    assert top <= 256
    # only vector stores write memory, and nothing in the run waits on a vector load
    text = "\n".join(lines)
    assert "global_load" not in text and "vmcnt" not in text and "scratch_" not in text and "buffer_" not in text
    if stores == "spread":  # the four checkpoint stores of a block at least 20 instructions apart
        top_i = next(n for n, ln in enumerate(lines) if ln.startswith(".Lphk_top_"))
        ins = [ln for ln in lines[top_i:] if not ln.endswith(":")]
        at = [n for n, ln in enumerate(ins) if ln.startswith("global_store_dwordx4")][:4]
        assert len(at) == 4 and min(b - a for a, b in zip(at, at[1:])) >= 20, at


def test_the_built_kernel_holds_the_run():
    """scripts/loop_report.py on the K = 16 float32 forward object: the run's block loop (from its top to its latch) is the all-hom
    trip of the generator, instruction for instruction, and the kernel has no scratch access."""
    obj = os.path.join(ROOT, "phlash_amd", "csrc", "build", "launch_fwd_f32_16.o")
    if not os.path.exists(obj):
        pytest.skip("no build directory (the library was built elsewhere)")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from loop_report import kernel_loops

    g = _generator()
    hom = g.trip_counts(g.build()[0])["all-hom"]
    k = kernel_loops(obj, "fwd_kernelIfLi16ELi1ELi8ELi4ELb1")
    assert len(k) == 1
    (info,) = k.values()
    assert info["scratch"] == 0
    rows = [r for r in info["loops"] if r["n"] == hom["total"] and r["pk"] == hom["packed"] and r["global"] == hom["stores"]]
    assert len(rows) == 1, [r["n"] for r in info["loops"]]
    assert rows[0]["scratch"] == 0 and rows[0]["nop"] == 0 and rows[0]["lds"] == 0 and rows[0]["waitcnt"] == 0


def test_no_other_forward_kernel_changed_registers():
    """The compiler's resource report of every kernel of the K = 16 float32 forward object against the recorded table
    (tests/golden/fwd_f32_16_resources.json: VGPRs, AGPRs, scratch bytes per lane, waves per SIMD).  The kernel with the run
    went from 204 to 256 VGPRs at the same 2 waves per SIMD when the run came.  The two- and eight-lane kernels were recorded anew
    when Group's masked lane reads became bit masks (tests/test_massless_fuzz.py): eight lanes 4 VGPRs fewer, two lanes 1 ... 2 more,
    no AGPR, no scratch, no kernel at fewer waves per SIMD than before; the other 20 kernels as they were."""
    import json
    import re

    log = os.path.join(ROOT, "phlash_amd", "csrc", "build", "launch_fwd_f32_16.o.log")
    if not os.path.exists(log):
        pytest.skip("no build directory (the library was built elsewhere)")
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "fwd_f32_16_resources.json")))
    keys = {"VGPRs": 0, "AGPRs": 1, "ScratchSize [bytes/lane]": 2, "Occupancy [waves/SIMD]": 3}
    got, cur = {}, None
    for line in open(log):
        m = re.search(r"remark:\s+([^:]+): (.+?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            cur = got.setdefault(v, [None] * 4)
        elif cur is not None and k in keys:
            cur[keys[k]] = int(v)
    assert got == want, {k: (want.get(k), got.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    run = got["_ZN3phk10fwd_kernelIfLi16ELi1ELi8ELi4ELb1EEEvNS_5KArgsE"]
    assert run[0] <= 256 and run[1] == 0 and run[2] == 0 and run[3] == 2  # no AGPR copies, no scratch, the parent's occupancy
