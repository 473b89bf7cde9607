"""Float64 / numpy restatement of care_sample_logits (include/care_hip.h; csrc/sample.hip), steps 1 - 5, one row at a time.

The integer hash is bit-exact.  s = x * inv_temperature is the fp32 product, as the kernel forms it (one IEEE
multiplication: the same bits everywhere), because the ORDER of s - ties included - defines the top-k set; everything after
it (exponentials, masses, logarithms, the Gumbel terms) is float64.  `sample_row` also reports how close each of the row's
three decisions was, so that a test can leave out rows that fp32 arithmetic may legitimately decide the other way:
  gumbel_margin   the gap between the two largest perturbed kept values (inf with one kept entry);
  nucleus_margin  the distance from top_p of the two cumulative masses on either side of the cut (the mass in front of the
                  last kept entry - unless that entry is the first, whose 0 is exact - and in front of the first dropped one);
  topk_margin     the gap between the k-th and the (k + 1)-th value in the order; 0 for exact duplicates, which the index
                  rule decides (identically here and in the kernel: the fp32 s are the same bits).
"""
import struct

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def fin(z: int) -> int:
    """The splitmix64 finaliser."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def h(a: int, n: int) -> int:
    return fin((a + GOLDEN * (n + 1)) & M64)


def h_vec(a, n: np.ndarray) -> np.ndarray:
    """h(a, n) for a uint64 array n and an int or uint64 array a (numpy's uint64 arithmetic wraps modulo 2^64)."""
    with np.errstate(over="ignore"):
        z = np.asarray(a, dtype=np.uint64) + np.uint64(GOLDEN) * (n.astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def row_state(seed: int, key: int, t: int) -> int:
    return h(seed & M64, ((key & 0xFFFFFFFF) << 16) | t)


def uniforms(seed: int, key: int, t: int, V: int) -> np.ndarray:
    """u_i = (2 k + 1) 2^-24, k the top 23 bits of h(h(seed, (key << 16) | t), i): exact, in (0, 1)."""
    k = h_vec(row_state(seed, key, t), np.arange(V, dtype=np.uint64)) >> np.uint64(41)
    return (2.0 * k.astype(np.float64) + 1.0) * 2.0 ** -24


def gumbels(seed: int, key: int, t: int, V: int) -> np.ndarray:
    return -np.log(-np.log(uniforms(seed, key, t, V)))


def f32(v) -> np.float32:
    return np.float32(v)


def pack_params(seed, temperature, top_k, top_p) -> bytes:
    """The kernel's 24-byte block: inv_temperature and top_p rounded to fp32."""
    return struct.pack("<Qffii", seed & M64, 1.0 / float(temperature), float(top_p), int(top_k), 0)


def sample_row(x, seed, key, t, temperature=1.0, top_k=0, top_p=1.0):
    """One row.  x: fp32 logits [V].  Returns a dict: tok, nkept, kept (indices in order), pmax, psum, logq, logp_model and
    the three margins."""
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[0]
    inv_t = f32(1.0 / float(temperature))
    top_p = float(f32(top_p))
    with np.errstate(invalid="ignore"):
        s32 = (x * inv_t).astype(np.float32) + f32(0.0)
    s = s32.astype(np.float64)
    idx = np.arange(V)
    order = np.lexsort((idx, -s))                       # s descending, index ascending
    order = order[np.isfinite(s[order]) | (s[order] == np.inf)]   # -inf: probability 0, never a candidate
    if order.size == 0:
        return dict(tok=0, nkept=0, kept=order, pmax=float(x[0]), psum=1.0, logq=0.0, logp_model=0.0,
                    gumbel_margin=np.inf, nucleus_margin=np.inf, topk_margin=np.inf)
    topk_margin = np.inf
    if 0 < top_k < V and top_k < order.size:
        topk_margin = float(s[order[top_k - 1]] - s[order[top_k]])
        order = order[:top_k]
    m = s[order[0]]
    nucleus_margin = np.inf
    if top_p < 1.0:
        e = np.exp(s[order] - m)
        q = e / e.sum()
        before = np.cumsum(q) - q
        before[0] = 0.0
        keep = before < top_p
        nk = int(keep.sum())
        assert keep[:nk].all()
        lo = top_p - before[nk - 1] if nk > 1 else np.inf
        hi = before[nk] - top_p if nk < order.size else np.inf
        nucleus_margin = float(min(lo, hi))
        order = order[:nk]
    g = gumbels(seed, key, t, V)
    val = s[order] + g[order]
    best = np.lexsort((order, -val))                    # value descending, index ascending
    tok = int(order[best[0]])
    gumbel_margin = float(val[best[0]] - val[best[1]]) if order.size > 1 else np.inf
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore"):
        psum = float(np.exp(x64 - x64[tok]).sum())
    logq = float(s[tok] - (m + np.log(np.exp(s[order] - m).sum())))
    return dict(tok=tok, nkept=int(order.size), kept=order, pmax=float(x[tok]), psum=psum, logq=logq, logp_model=-np.log(psum),
                gumbel_margin=gumbel_margin, nucleus_margin=nucleus_margin, topk_margin=topk_margin)


def sample_rows(x, seed, keys, t, temperature=1.0, top_k=0, top_p=1.0):
    """sample_row over the rows of x [rows, V] (keys None: the row index); a dict of arrays."""
    rows = [sample_row(x[r], seed, r if keys is None else int(keys[r]), t, temperature, top_k, top_p) for r in range(x.shape[0])]
    out = {k: np.array([r[k] for r in rows]) for k in rows[0] if k != "kept"}
    out["kept"] = [r["kept"] for r in rows]
    return out
