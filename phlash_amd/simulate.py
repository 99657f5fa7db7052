"""Posterior predictive simulation: replicate observation rows drawn on the GPU from the models of a ``fit()`` sample, under
the data's own accessibility mask (``phk_simulate``, defined in ``include/phlash_hip.h``).

``simulate``         the thin tensor wrapper of the C call: allocates the outputs that are asked for and nothing else;
``simulate_rows``    replicate rows (and hidden paths) of whole contigs under one or several ``DemographicModel``;
``replicate_check``  the posterior predictive check: het counts per bin and the length spectrum of hom runs of the data
                     against their distribution over models x replicates, from the kernel's on-the-fly statistics -- no
                     replicate row is ever stored.

There is no CPU path: the draws come from the HIP kernel or not at all.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .data import RawContig
from .params import PSMCParams
from .size_history import DemographicModel

ROW_ALIGN = 16  # phk_simulate stores 16 bytes per lane: row strides are padded to it (torch allocations are aligned far beyond)
DEFAULT_STAT_BYTES = 256 << 20  # replicate_check's cap on the device buffers of one kernel call


class SimOut(NamedTuple):
    obs: torch.Tensor | None    # int8 [B, S, n_rep, L]
    paths: torch.Tensor | None  # uint8 [B, S, n_rep, L]
    het: torch.Tensor | None    # int32 [B, S, n_rep, ceil(L / bin)]
    runs: torch.Tensor | None   # int32 [B, S, n_rep, 32]
    flags: torch.Tensor         # int32 [1] on the device: bit 0 = a draw had no mass (not synchronised here)


class Simulated(NamedTuple):
    obs: object    # int8 [B, S, n_rep, L] on the device (a list of such tensors, one per contig, for a list of contigs)
    paths: object  # uint8, same shapes, or None


class ReplicateCheck(NamedTuple):
    het_data: object   # [N, nbin] hets per bin of the data
    het_mean: object   # mean over models x replicates
    het_lo: object     # 2.5 % quantile
    het_hi: object     # 97.5 % quantile
    het_p: object      # share of (model, replicate) pairs whose count is >= the data's
    runs_data: object  # [N, 32] histogram over floor(log2(length)) of the data's runs of hom windows
    runs_mean: object
    runs_lo: object
    runs_hi: object
    runs_p: object


def simulate(params: torch.Tensor, L: int, n_rep: int = 1, seed: int = 0, S: int | None = None, mask: torch.Tensor | None = None,
             seq0: int = 0, obs: bool = True, paths: bool = False, bin: int | None = None, runs: bool = False) -> SimOut:
    """``params``: float64 [B, S or 1, 7, K] on the GPU (rows b,d,u,v,emis0,emis1,pi); a second dimension of 1 is one block
    per particle, broadcast over the S rows (``S``, or the mask's rows, or 1).  ``mask``: int8 [S, >= L] on the same device,
    negative = missing.  ``bin``: ask for het counts per ``bin`` sites.  Stream-ordered; nothing is synchronised."""
    assert params.is_cuda and params.dtype == torch.float64 and params.ndim == 4 and params.shape[2] == 7, "params: float64 [B, S or 1, 7, K] on the GPU"
    dev = params.device
    B, Sp, _, K = params.shape
    if mask is not None:
        assert mask.dtype == torch.int8 and mask.ndim == 2 and mask.device == dev, "mask: int8 [S, >= L] on the parameters' device"
        if mask.stride(1) != 1:
            mask = mask.contiguous()
    if S is None:
        S = mask.shape[0] if mask is not None else Sp
    assert Sp in (1, S) and (mask is None or mask.shape[0] == S), "params, mask and S disagree on the number of rows"
    if params.stride(3) != 1 or params.stride(2) != K:
        params = params.contiguous()
    stride = -(-int(L) // ROW_ALIGN) * ROW_ALIGN
    nbin = -(-int(L) // int(bin)) if bin is not None else 0
    o = torch.empty((B, S, n_rep, stride), dtype=torch.int8, device=dev) if obs else None
    p = torch.empty((B, S, n_rep, stride), dtype=torch.uint8, device=dev) if paths else None
    h = torch.empty((B, S, n_rep, nbin), dtype=torch.int32, device=dev) if bin is not None else None
    r = torch.empty((B, S, n_rep, 32), dtype=torch.int32, device=dev) if runs else None
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = _lib.load().phk_simulate(
        dev.index, K, params.data_ptr(), params.stride(0), 0 if Sp == 1 else params.stride(1), B, S, int(n_rep), int(L),
        ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(seq0), ptr(mask), mask.stride(0) if mask is not None else 0,
        ptr(o), ptr(p), stride, int(bin) if bin is not None else 1, ptr(h), ptr(r), flags.data_ptr(), ctypes.c_void_p(stream))
    _lib.check(rc)
    return SimOut(o[..., :L] if obs else None, p[..., :L] if paths else None, h, r, flags)


def _blocks(dms, window_size, dev):
    """[B, 1, 7, K] float64 on the device: one block per model, theta and rho per window"""
    per = [DemographicModel(eta=m.eta, theta=float(m.theta) * window_size, rho=float(m.rho) * window_size) for m in dms]
    pps = [PSMCParams.from_dm(m) for m in per]
    return torch.stack([torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for f in PSMCParams._fields]) for p in pps])[:, None].to(dev)


def _models(dms):
    single = isinstance(dms, DemographicModel)
    dms = [dms] if single else list(dms)
    assert len(dms) > 0, "no model to simulate under"
    assert all(m.M == dms[0].M for m in dms), "all models must have the same number of states"
    return dms


def _device(device):
    dev = torch.device(device if device is not None else "cuda")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _data_rows(data, window_size):
    from .decode import _rows

    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    return _rows(data)


def _raise_on(flags):
    if int(flags.item()) & 1:
        raise FloatingPointError("phk_simulate: a draw had no mass (a transition row, pi or an emission row is zero or not finite)")


def simulate_rows(dms, data=None, n_sites: int | None = None, n_rep: int = 1, seed: int = 0, window_size: int = 100, paths: bool = False,
                  device=None) -> Simulated:
    """Replicate rows drawn from each model: ``Simulated(obs, paths)``.

    dms: one ``DemographicModel`` or the list ``fit()`` returns (B models), theta and rho per base pair, evaluated per window as
        in ``posterior_tmrca``.
    data: int8 [N, L] het matrix, or a list of ``RawContig`` (or matrices) of different lengths.  Every row lends its missing
        windows to its replicates (S = N); a list is padded with missing windows and cut again per contig.  Without ``data``
        there is one unmasked row of ``n_sites`` windows.
    Returns ``obs`` int8 [B, S, n_rep, L] on the device (codes -1 / 0 / 1), and with ``paths=True`` the hidden states, uint8 of
    the same shape; for a list of contigs, lists with one tensor [B, rows, n_rep, length] per contig.  The same ``seed`` gives
    the same bytes; replicate r does not depend on ``n_rep``."""
    dms = _models(dms)
    dev = _device(device)
    if data is None:
        assert n_sites is not None and n_sites >= 1, "without data, n_sites is required"
        out = simulate(_blocks(dms, window_size, dev), int(n_sites), n_rep=n_rep, seed=seed, S=1, paths=paths)
        _raise_on(out.flags)
        return Simulated(out.obs, out.paths)
    rows, spans = _data_rows(data, window_size)
    mask = torch.as_tensor(rows).to(dev)
    out = simulate(_blocks(dms, window_size, dev), rows.shape[1], n_rep=n_rep, seed=seed, mask=mask, paths=paths)
    _raise_on(out.flags)
    if spans is None:
        return Simulated(out.obs, out.paths)
    cut = lambda x: None if x is None else [x[:, r : r + n, :, :length] for r, n, length in spans]  # noqa: E731
    return Simulated(cut(out.obs), cut(out.paths))


def data_statistics(rows: np.ndarray, bin: int):
    """(het [N, nbin], runs [N, 32]) int64 of an int8 matrix (-1 missing, 0 hom, >= 1 het), on the host: the kernel's two
    statistics of the data's own rows"""
    rows = np.asarray(rows)
    N, L = rows.shape
    nbin = -(-L // bin)
    pad = np.zeros((N, nbin * bin), dtype=np.int64)
    pad[:, :L] = rows >= 1
    het = pad.reshape(N, nbin, bin).sum(2)
    runs = np.zeros((N, 32), dtype=np.int64)
    for i in range(N):
        hom = np.concatenate([[0], (rows[i] == 0).astype(np.int8), [0]])
        edge = np.flatnonzero(np.diff(hom))
        length = edge[1::2] - edge[0::2]
        if length.size:
            runs[i] = np.bincount(np.floor(np.log2(length)).astype(int), minlength=32)[:32]
    return het, runs


def replicate_check(dms, data, n_rep: int = 100, bin: int = 100, seed: int = 0, window_size: int = 100, device=None,
                    max_stat_bytes: int = DEFAULT_STAT_BYTES) -> ReplicateCheck:
    """Posterior predictive check of the het counts per bin of ``bin`` windows and of the length spectrum of runs of hom
    windows (32 buckets by floor(log2(length))), for every row of ``data``.

    ``n_rep`` replicates of every row are drawn under every model with the row's own missing windows, and reduced inside the
    kernel: no row is stored.  For each statistic ``mean``, ``lo`` and ``hi`` are the mean and the 2.5 % and 97.5 % quantiles over
    models x replicates and ``p`` the share of (model, replicate) pairs whose statistic is >= the data's.  The data's own
    statistics are computed on the host.  One kernel call's statistic buffers stay below ``max_stat_bytes`` (default 256 MiB):
    the models are cut into slabs, which changes no draw; the slabs' counts are gathered on the host, where the quantiles
    are taken.  Returns float64 arrays [N, nbin] / [N, 32] on the host (integer for the data's); for a list of contigs, lists
    with one array per contig, cut to the contig's bins."""
    dms = _models(dms)
    dev = _device(device)
    rows, spans = _data_rows(data, window_size)
    N, L = rows.shape
    nbin = -(-L // bin)
    mask = torch.as_tensor(rows).to(dev)
    blocks = _blocks(dms, window_size, dev)
    B = len(dms)
    per_model = N * n_rep * (nbin + 32) * 4
    slab = max(1, min(B, int(max_stat_bytes) // per_model))
    het = np.empty((B, N, n_rep, nbin), dtype=np.int32)
    runs = np.empty((B, N, n_rep, 32), dtype=np.int32)
    for b0 in range(0, B, slab):
        out = simulate(blocks[b0 : b0 + slab], L, n_rep=n_rep, seed=seed, mask=mask, seq0=b0 * N, obs=False, bin=bin, runs=True)
        het[b0 : b0 + slab] = out.het.cpu().numpy()
        runs[b0 : b0 + slab] = out.runs.cpu().numpy()
        _raise_on(out.flags)
    het_data, runs_data = data_statistics(rows, bin)

    def summary(sim, dat):  # sim [B, N, n_rep, m], dat [N, m]
        x = np.moveaxis(sim, 1, 0).reshape(N, B * n_rep, -1)
        lo, hi = np.quantile(x, [0.025, 0.975], axis=1)
        return x.mean(1), lo, hi, (x >= dat[:, None, :]).mean(1)

    fields = (het_data,) + summary(het, het_data) + (runs_data,) + summary(runs, runs_data)
    if spans is not None:
        cut = lambda x, bins: [x[r : r + n, : (-(-length // bin) if bins else 32)] for r, n, length in spans]  # noqa: E731
        fields = tuple(cut(x, i < 5) for i, x in enumerate(fields))
    return ReplicateCheck(*fields)
