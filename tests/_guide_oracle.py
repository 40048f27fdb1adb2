"""CPU oracle of the guidance stage (csrc/guide.hip): float64 numpy from the 16-bit bits, written from the contract.
No transformers import here: the comparison with HF's class lives in tests/test_guide_oracle.py.

One pair (conditional row x_c, negative row x_u, gamma fp32, log_beta fp32 <= 0), T the storage type:
    lse       = max + log(sum exp(x_i - max))                          (double)
    c_i, u_i  = x_c[i] - lse_c, x_u[i] - lse_u
    g_i       = gamma * (c_i - u_i) + u_i                               (double, every operation rounded on its own)
    out_i     = T(g_i), ONE rounding (round to odd to fp32, then nearest even); a finite g_i beyond T's range -> the largest finite
    cut       : log_beta > -inf: out_i = -inf unless f32(x_c[i]) - f32(max x_c) >= log_beta   (exact fp32 difference)
    non-finite: x_c[i] -inf / NaN -> -inf;  x_u[i] non-finite with x_c[i] finite -> T(c_i);  lse_c or lse_u non-finite -> row of -inf
The device's exp / log differ from numpy's in the last place, so an element whose float64 g_i lies within
BAND * (|gamma| + |1 - gamma|) of a 16-bit rounding midpoint may come out as the adjacent code (`Guided.band`, `Guided.alt`); the
census of tests/test_guide_oracle.py caps how many such elements the GPU test's cases hold.

The second half builds the cases of tests/test_guide_gpu.py's door test, so that the CPU census runs over exactly those."""
import numpy as np

BAND = 1e-9
CAP = 1e-4                   # the largest share of in-band elements (census) / of elements that took the adjacent code (GPU)
GAMMAS = (0.0, 0.5, 1.0, 1.5, 3.0)
VOCABS = (1, 2, 63, 64, 65, 1000, 32768, 32769, 131075)


# ---- the two storage types as bits ----
def to_f64(bits, bf16: bool) -> np.ndarray:
    b = np.asarray(bits, np.uint16)
    if bf16:
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return b.view(np.float16).astype(np.float64)


def inf_bits(bf16: bool) -> int:
    return 0x7f80 if bf16 else 0x7c00


def f64_to_f32_odd(d: np.ndarray) -> np.ndarray:
    """double -> float rounded to odd: truncate toward zero, then set the last bit when inexact."""
    d = np.asarray(d, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = d.astype(np.float32)
    df = f.astype(np.float64)
    exact = (df == d) | np.isnan(d)
    b = f.view(np.uint32).copy()
    with np.errstate(invalid="ignore"):
        away = ~exact & (np.abs(df) > np.abs(d))
    b[away] -= 1
    b[~exact] |= 1
    return b.view(np.float32)


def f32_to_bits_rne(f: np.ndarray, bf16: bool) -> np.ndarray:
    f = np.asarray(f, np.float32)
    if not bf16:
        with np.errstate(over="ignore"):
            return f.astype(np.float16).view(np.uint16)
    b = f.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(f)
    r[nan] = ((b[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def round16(g, bf16: bool) -> np.ndarray:
    """FINITE float64 values rounded once to the storage type, saturating at the largest finite magnitude -> bits."""
    b = f32_to_bits_rne(f64_to_f32_odd(g), bf16)
    sat = (b & 0x7fff) == inf_bits(bf16)
    b[sat] -= 1
    return b


def from_f64(x, bf16: bool) -> np.ndarray:
    """float64 values (infinities and NaN included) -> bits, round to nearest even."""
    x = np.asarray(x, np.float64)
    b = f32_to_bits_rne(f64_to_f32_odd(x), bf16)
    inf = np.isinf(x)
    b[inf] = np.where(x[inf] > 0, inf_bits(bf16), 0x8000 | inf_bits(bf16)).astype(np.uint16)
    return b


def _step(bits: np.ndarray, up: np.ndarray) -> np.ndarray:
    """The adjacent 16-bit code above (up) / below each code, through the order-preserving keys."""
    b = bits.astype(np.int64)
    key = np.where(b & 0x8000, ~b & 0xffff, b | 0x8000)
    key = key + np.where(up, 1, -1)
    return np.where(key & 0x8000, key & 0x7fff, ~key & 0xffff).astype(np.uint16)


# ---- the contract ----
def lse(x: np.ndarray) -> float:
    """max + log(sum exp(x - max)) of a float64 row; NaN for a NaN element, a +inf maximum or a row of -inf."""
    x = np.asarray(x, np.float64)
    if np.isnan(x).any():
        return float("nan")
    m = x.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(m + np.log(np.exp(x - m).sum()))


class Guided:
    """One guided row: out (bits), g (float64, the un-rounded value where one was computed, else NaN), band (elements within the
    excuse band of a rounding midpoint), alt (the adjacent code such an element may take instead)."""

    def __init__(self, out, g, band, alt):
        self.out, self.g, self.band, self.alt = out, g, band, alt


def guide_pair(xc_bits, xu_bits, gamma, log_beta, bf16: bool, lse_c=None, lse_u=None) -> Guided:
    neg_inf = np.uint16(0x8000 | inf_bits(bf16))
    xc, xu = to_f64(xc_bits, bf16), to_f64(xu_bits, bf16)
    V = xc.shape[0]
    gamma = float(np.float32(gamma))
    lb = np.float32(log_beta)
    lse_c = lse(xc) if lse_c is None else lse_c
    lse_u = lse(xu) if lse_u is None else lse_u
    out = np.full(V, neg_inf, np.uint16)
    g = np.full(V, np.nan)
    band = np.zeros(V, bool)
    alt = out.copy()
    if not (np.isfinite(lse_c) and np.isfinite(lse_u)):
        return Guided(out, g, band, alt)
    live = np.isfinite(xc)
    if lb > -np.inf:
        x32 = xc.astype(np.float32)
        with np.errstate(invalid="ignore"):
            live &= (x32 - np.fmax.reduce(x32)) >= lb
    c = xc - lse_c
    with np.errstate(invalid="ignore"):
        u = xu - lse_u
        both = gamma * (c - u) + u
    g[live] = np.where(np.isfinite(xu), both, c)[live]
    out[live] = round16(g[live], bf16)
    # the excuse band: |g - midpoint| <= BAND * (|gamma| + |1 - gamma|), the midpoint between out and the code on g's other side
    v = to_f64(out[live], bf16)
    other = _step(out[live], g[live] > v)
    w = to_f64(other, bf16)
    tol = BAND * (abs(gamma) + abs(1 - gamma))
    with np.errstate(invalid="ignore"):
        near = np.isfinite(w) & (g[live] != v) & (np.abs(g[live] - (v + w) / 2) <= tol)
    band[live] = near
    alt[live] = np.where(near, other, out[live])
    return Guided(out, g, band, alt)


def log_softmax16(x_bits, bf16: bool) -> np.ndarray:
    """The once-rounded log_softmax of a row with a finite log-sum-exp (-inf stays -inf) -> bits."""
    x = to_f64(x_bits, bf16)
    out = np.full(x.shape[0], 0x8000 | inf_bits(bf16), np.uint16)
    fin = np.isfinite(x)
    out[fin] = round16(x[fin] - lse(x), bf16)
    return out


def guide_rows(x_bits, vocab: int, cond, neg, scale, log_beta, bf16: bool, lse_cache=None):
    """The door on a whole matrix x_bits [rows, ld]: (the matrix afterwards, band mask, adjacent codes), all [rows, ld]."""
    y = np.array(x_bits, np.uint16, copy=True)
    band = np.zeros(y.shape, bool)
    alt = y.copy()
    for p in range(len(cond)):
        c, u = int(cond[p]), int(neg[p])
        kw = {}
        if lse_cache is not None:
            for r in (c, u):
                if r not in lse_cache:
                    lse_cache[r] = lse(to_f64(x_bits[r, :vocab], bf16))
            kw = dict(lse_c=lse_cache[c], lse_u=lse_cache[u])
        res = guide_pair(x_bits[c, :vocab], x_bits[u, :vocab], scale[p], log_beta[p], bf16, **kw)
        y[c, :vocab], band[c, :vocab] = res.out, res.band
        alt[c] = y[c]
        alt[c, :vocab] = res.alt
    return y, band, alt


def first_argmax_bits(bits, bf16: bool) -> int:
    """argmax_rows_lp's rule on a row of bits: the first index of the largest number; NaN and -inf never win; 0 when nothing does."""
    x = to_f64(bits, bf16)
    ok = ~np.isnan(x) & (x > -np.inf)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (x == x[ok].max()))[0])


# ---- the cases of the door test (tests/test_guide_gpu.py) and of the census (tests/test_guide_oracle.py) ----
COND = (0, 3, 4, 7, 8)       # cond_row < neg_row and cond_row > neg_row mixed; rows 10 and 11 are in no pair
NEG = (1, 2, 5, 6, 9)
ROWS = 12
CANARY = 0x3555              # columns [vocab, ld) of every row
BOUNDARY_LOG_BETA = -2.0


def _row(kind: str, V: int, rng, bf16: bool) -> np.ndarray:
    big = -3.0e38 if bf16 else -60000.0
    x = rng.normal(0.0, 3.0, V)
    if kind == "peaked":
        x = rng.normal(0.0, 1.0, V)
        x[int(rng.integers(V))] += 12.0
    elif kind == "flat":
        x[:] = 1.5
    elif kind == "masked":
        x[rng.random(V) < 0.3] = -np.inf
        x[0] = 0.25
    elif kind == "nan":
        x[V // 2] = np.nan
    elif kind == "allinf":
        x[:] = -np.inf
    elif kind == "saturate":          # one element so far below the rest that gamma * (c - u) leaves the storage type's range
        x[0] = big
    elif kind == "boundary":          # the maximum 4.0, one element exactly 2.0 below it (kept at log_beta = -2), one an ulp lower (dropped)
        x = np.minimum(x, 3.0)
        x[0] = 4.0
        if V > 1:
            x[1] = 2.0
        if V > 2:
            x[2] = to_f64(_step(from_f64(np.float64([2.0]), bf16), np.array([False])), bf16)[0]
    return from_f64(x, bf16)


SCENE_A = (("random", "random"), ("peaked", "random"), ("flat", "peaked"), ("masked", "random"), ("random", "masked"))
SCENE_B = (("nan", "random"), ("random", "allinf"), ("saturate", "random"), ("masked", "masked"), ("boundary", "random"))


def scene(name: str, V: int, bf16: bool) -> np.ndarray:
    """x_bits [ROWS, V + 3] of scene 'A' / 'B': the pairs' rows, two unpaired rows (random, nan), canaries behind column V."""
    rng = np.random.default_rng(1000003 * V + 17 * (name == "B") + bf16)
    x = np.full((ROWS, V + 3), CANARY, np.uint16)
    for p, (kc, ku) in enumerate(SCENE_A if name == "A" else SCENE_B):
        x[COND[p], :V] = _row(kc, V, rng, bf16)
        x[NEG[p], :V] = _row(ku, V, rng, bf16)
    x[10, :V] = _row("random", V, rng, bf16)
    x[11, :V] = _row("nan", V, rng, bf16)
    return x


def launches(name: str):
    """The (scale[5], log_beta[5]) records of a scene's launches: scene A every rotation of GAMMAS over the pairs for beta off, 0.1
    and 1; scene B every rotation with the pairs' own cuts (the boundary pair at exactly -2)."""
    out = []
    with np.errstate(divide="ignore"):
        betas = [np.float32(np.log(np.float64(b))) for b in (0.0, 0.1, 1.0)]
    for r in range(5):
        sc = np.float32([GAMMAS[(p + r) % 5] for p in range(5)])
        if name == "A":
            out += [(sc, np.full(5, lb, np.float32)) for lb in betas]
        else:
            out.append((sc, np.float32([-np.inf, betas[1], -np.inf, betas[2], BOUNDARY_LOG_BETA])))
    return out
