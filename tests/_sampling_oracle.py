"""CPU oracle of the sampled decode (HF 4.31 generate(do_sample=True)) and of its Philox4x32-10 stream.

Steps, for one row of fp16 / bf16 logits x:
  1. s = dtype(float32(x) / float32(t))                      (torch's rounding of `half_tensor / t`)
  2. top-k: keep s >= the k-th largest s (all ties kept); k = 0 off, k clamped to [1, V]
  3. top-p (top_p < 1): p = softmax(s) over the top-k set; keep iff the mass of kept tokens with a strictly greater score
     is < top_p; the maximal score is always kept
  4. the smallest kept index, in vocabulary order, whose inclusive prefix mass exceeds u * Z (Z = kept mass)
Masses are exp(s - max s), 1 where s equals the maximum (also when it is infinite).  Everything here is float64, except that
s - max s is taken in float32 like the kernel."""
from __future__ import annotations

import numpy as np
import torch

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c = [int(v) & M32 for v in ctr]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
    return c


def uniform(seed: int, step: int, stream: int = 0) -> float:
    """u of one draw: counter (step, stream lo, stream hi, 0), key (seed lo, seed hi); (x0 >> 8) * 2^-24, exact in fp32."""
    seed, stream = int(seed) & ((1 << 64) - 1), int(stream) & ((1 << 64) - 1)
    x0 = philox4x32_10([step, stream & M32, stream >> 32, 0], [seed & M32, seed >> 32])[0]
    return (x0 >> 8) * 2.0 ** -24


def scaled_scores(x: torch.Tensor, t: float) -> np.ndarray:
    """Step 1 on a 1-D fp16 / bf16 tensor: float64 scores (NaN -> -inf)."""
    s = x if float(np.float32(t)) == 1.0 else (x.float() / torch.tensor(t, dtype=torch.float32)).to(x.dtype)
    s = s.double().numpy()
    return np.where(np.isnan(s), -np.inf, s)


def masses(s: np.ndarray) -> np.ndarray:
    m = s.max()
    with np.errstate(invalid="ignore", over="ignore"):
        d = (s.astype(np.float32) - np.float32(m)).astype(np.float64)
        e = np.exp(d)
    return np.where(s == m, 1.0, np.where(np.isnan(e), 0.0, e))


def kept(s: np.ndarray, top_k: int, top_p: float):
    """Steps 2-3: (kept mask, smallest |G - top_p * Z_k| / Z_k over the top-k set — the top-p boundary distance; inf when
    top-p is off)."""
    V = s.shape[0]
    keep = np.ones(V, bool)
    if top_k and top_k > 0:
        k = min(max(int(top_k), 1), V)
        kth = np.partition(s, V - k)[V - k]
        keep = s >= kth
    dist = np.inf
    if top_p is not None and np.float32(top_p) < 1:
        p = np.float64(np.float32(top_p))
        w = masses(s) * keep
        Z = w.sum()
        order = np.argsort(-s, kind="stable")
        ss, cs = s[order], np.concatenate([[0.0], np.cumsum(w[order])])
        G = cs[np.searchsorted(-ss, -s, side="left")]      # mass of the tokens with a strictly greater score
        keep = keep & ((G < p * Z) | (s == s.max()))
        cand = (w > 0) & (s != s.max())                     # (the maximal score is kept whatever G is)
        dist = float(np.min(np.abs(G[cand] - p * Z)) / Z) if cand.any() else np.inf
    return keep, dist


def draw(s: np.ndarray, keep: np.ndarray, u: float):
    """Step 4: (token, distance of u*Z to the nearest prefix-mass boundary / Z)."""
    w = masses(s) * keep
    c = np.cumsum(w)
    Z = c[-1]
    target = u * Z
    tok = int(np.searchsorted(c, target, side="right"))
    tok = min(tok, len(s) - 1)
    bounds = c[keep]
    return tok, float(np.min(np.abs(bounds - target)) / Z)


def sample_row(x: torch.Tensor, t: float, top_k: int, top_p, u: float):
    """The whole chain on one row: dict(token, n_kept, p_dist, u_dist, q = the kept distribution)."""
    s = scaled_scores(x, t)
    keep, p_dist = kept(s, top_k, top_p)
    tok, u_dist = draw(s, keep, u)
    w = masses(s) * keep
    return dict(token=tok, n_kept=int(keep.sum()), p_dist=p_dist, u_dist=u_dist, q=w / w.sum())
