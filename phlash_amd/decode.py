"""Posterior decoding of whole contigs: the posterior mean TMRCA along the genome (what ``psmc -d`` reports), under one
fitted model or averaged over the posterior sample ``fit`` returns.

The HMM posteriors come from the decode sweep of the HIP engine (``PSMCKernel.posterior`` -> ``phk_posterior``); this
module only builds the models, pads ragged inputs and averages.  There is no CPU path.
"""

from __future__ import annotations

import numpy as np
import torch

from .data import RawContig
from .kernel import PSMCKernel
from .params import PSMCParams
from .size_history import DemographicModel


def _rows(data):
    """-> (int8 [N, Lmax] padded with -1, list of (first row, rows, length) per contig, or None for a plain matrix)"""
    if isinstance(data, (list, tuple)):
        mats = []
        for c in data:
            m = c.het_matrix if isinstance(c, RawContig) else c
            m = np.asarray(m)
            mats.append(m[None] if m.ndim == 1 else m)
        Lmax = max(m.shape[1] for m in mats)
        out = np.full((sum(m.shape[0] for m in mats), Lmax), -1, dtype=np.int8)
        spans, r = [], 0
        for m in mats:
            out[r : r + m.shape[0], : m.shape[1]] = m
            spans.append((r, m.shape[0], m.shape[1]))
            r += m.shape[0]
        return out, spans
    if isinstance(data, torch.Tensor):
        data = data.cpu().numpy()
    d = np.asarray(data)
    assert d.ndim == 2 and d.dtype == np.int8, "data: int8 [N, L] het matrix (or a list of RawContig)"
    return d, None


def posterior_tmrca(dms, data, window_size: int = 100, bin: int = 1, device=None, double_precision: bool = False):
    """Posterior mean TMRCA per bin of ``bin`` windows, for every row of ``data``.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, with theta and rho per base pair; every model is evaluated
        with theta and rho times ``window_size`` (per window) and the states' expected coalescence times ``dm.eta.ect()``,
        in the model's own time unit (generations when ``fit`` was given ``mutation_rate``), and the tracks are averaged
        with equal weight.
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of
        int8 matrices) of different lengths: they are padded with missing windows and the padding is stripped again.
    Returns float64 [N, ceil(L / bin)] on the device for a matrix, a list of such tensors (one per contig) for a list.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    values = torch.stack([torch.as_tensor(dm.eta.ect(), dtype=torch.float64) for dm in dms]).to(dev)  # [B, M]
    inds = torch.arange(rows.shape[0], device=dev)
    out = kern.posterior(pp, inds, values=values, bin=bin, marginals=False)
    track = out.mean.to(torch.float64).mean(0)  # [N, nbin]: equal weight per model
    if spans is None:
        return track
    return [track[r : r + n, : (length + bin - 1) // bin] for r, n, length in spans]
