"""CPU oracle of the further warpers of the sampled decode: min-p -> typical-p -> epsilon -> eta on the kept set
that top-k / top-p (tests/_sampling_oracle.py) left, float64 numpy.

Every stage sees the kept set K of the stage before it and p_i = m_i / Z_K, with
  m_i = round(exp(l_i) * 2^40), l_i = float32(s_i) - float32(max s)   (the kernel's fixed-point masses; 2^40 at the row's maximum)
and a token whose mass rounds to 0 takes part in no sum:
  min-p      keep iff m_i >= min_p * m_max(K)
  typical-p  mu = sum_K m_i l_i / Z, d_i = |l_i - mu|; keep iff the mass of the tokens of K with a strictly smaller d is < typical_p * Z
  epsilon    keep iff m_i >= eps * Z
  eta        H = ln(Z / 2^40) - mu, eta = min(eps, sqrt(eps) * exp(-H)); keep iff m_i >= eta * Z
The largest score of K always stays.  Next to the kept mask the oracle returns the smallest margin of every comparison it made: a
mass against a threshold relative to the threshold, a (non-empty) strictly-smaller mass against typical_p * Z relative to Z, a
distance d against the threshold distance in nats.  A row whose margin is below MARGIN may legitimately come out differently on the device."""
from __future__ import annotations

import numpy as np

from tests import _sampling_oracle as S

# The device masses carry up to 2^-23 relative error (fp32 expf, then the 2^-40 rounding) and |l| <= 28.4 wherever a mass is not
# zero, so E_p[l] and H are good to about 3.4e-6 nats; 1e-5 covers that and the 1e-6 the top-p boundary already uses.
MARGIN = 1e-5
ONE = float(2 ** 40)


def fixed_masses(s: np.ndarray) -> np.ndarray:
    """The 2^-40 fixed-point masses as float64 integers (exact: each is <= 2^40)."""
    return np.rint(S.masses(s) * ONE)


def ell(s: np.ndarray) -> np.ndarray:
    """l_i = s_i - max s, the subtraction in float32 like key_mass; 0 at the maximum also when it is infinite."""
    m = s.max()
    with np.errstate(invalid="ignore", over="ignore"):
        d = (s.astype(np.float32) - np.float32(m)).astype(np.float64)
    return np.where(s == m, 0.0, d)


def _f32(v) -> float:
    return float(np.float32(v))


def _floor(s, keep, m, thr, margins, name):
    """keep iff m >= thr, the largest score of `keep` always."""
    top = s == s[keep].max()
    cand = keep & ~top
    if cand.any():
        margins[name] = min(margins.get(name, np.inf), float(np.min(np.abs(m[cand] - thr)) / thr))
    return keep & ((m >= thr) | top)


def _sums(keep, m, l):
    w = keep & (m > 0)
    Z = float(m[w].sum())
    return Z, float((m[w] * l[w]).sum()) / Z


def warp(s: np.ndarray, keep: np.ndarray, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """s: float64 scores (tests/_sampling_oracle.scaled_scores), keep: the mask top-k / top-p left -> (kept mask, margins), margins
    a dict stage -> the smallest margin of that stage's comparisons (absent: the stage compared nothing)."""
    keep = keep.copy()
    m, l = fixed_masses(s), ell(s)
    margins = {}
    min_p, typical_p, eps, eta_c = _f32(min_p), _f32(typical_p), _f32(epsilon_cutoff), _f32(eta_cutoff)
    if min_p > 0:
        keep = _floor(s, keep, m, min_p * ONE, margins, "min_p")       # the maximum of the row is in K: max_K m = 2^40
    if typical_p < 1:
        Z, mu = _sums(keep, m, l)
        with np.errstate(invalid="ignore"):
            d = np.abs(l - mu)                                          # inf where the score is -inf
        idx = np.flatnonzero(keep)
        order = idx[np.argsort(d[idx], kind="stable")]
        ds = d[order]
        cs = np.concatenate([[0.0], np.cumsum(m[order])])
        G = np.empty_like(d)
        G[order] = cs[np.searchsorted(ds, ds, side="left")]             # the mass of the tokens of K with a strictly smaller d
        pos = keep & (m > 0)
        new = keep.copy()
        new[idx] = G[idx] < typical_p * Z
        cmp = pos & (G > 0)                                             # (G = 0 is an empty sum on both sides: the smallest d always stays)
        if cmp.any():
            margins["typical_mass"] = float(np.min(np.abs(G[cmp] - typical_p * Z)) / Z)
        D = d[new & pos].max()                                          # the threshold distance
        other = keep & np.isfinite(d) & (d != D)
        if other.any():
            margins["typical_d"] = float(np.min(np.abs(d[other] - D)))
        keep = new
    if eps > 0:
        Z, _ = _sums(keep, m, l)
        keep = _floor(s, keep, m, eps * Z, margins, "epsilon")
    if eta_c > 0:
        Z, mu = _sums(keep, m, l)
        H = np.log(Z / ONE) - mu
        eta = min(eta_c, np.sqrt(eta_c) * np.exp(-H))
        keep = _floor(s, keep, m, eta * Z, margins, "eta")
    return keep, margins


def margin(margins: dict) -> float:
    return min(margins.values(), default=np.inf)


def warp_row(x, t: float, top_k: int, top_p, u: float, **warpers):
    """The whole chain on one fp16 / bf16 row (a torch tensor): dict(keep, n_kept, token, margin = the smallest margin of the
    top-p boundary and the four stages, u_dist, q = the kept distribution)."""
    s = S.scaled_scores(x, t)
    k0, p_dist = S.kept(s, top_k, top_p)
    keep, mg = warp(s, k0, **warpers)
    tok, u_dist = S.draw(s, keep, u)
    w = S.masses(s) * keep
    # (the top-p boundary keeps its own limit of 1e-6: rescaled so that one comparison against MARGIN serves both)
    return dict(keep=keep, n_kept=int(keep.sum()), token=tok, margin=min(margin(mg), p_dist * (MARGIN / 1e-6)), u_dist=u_dist,
                q=w / w.sum())
