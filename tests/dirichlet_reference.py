"""The Dirichlet stream of corrla_dirichlet_draws_* / corrla_dirichlet_sample_* restated in numpy, from the text of the header
comment of corrla_rs_amd/csrc/dirichlet_kernels.hpp and of include/corrla_rsvd.h (THE STREAM) -- not from any other code:
Philox4x32-10 in uint64 arithmetic, the 53-bit uniforms, Box-Muller (cosine branch), the three gamma methods with their
attempt loops, the row, the box test and the shot / stop rule.  Vectorised over the draws; every operation is one float64
operation in the documented order.

Besides the rows `draws` returns what the GPU tests need to know about their own seeds:
  margin   per draw, the smallest distance of any attempt from a decision the device could take the other way: |w| for the
           test w <= 0, and |0.5 z2 + D ((1 - v) + log v) - log q| for the acceptance (the squeeze accepts only what the
           logarithmic test accepts too, so it cannot change an outcome).  inf for alpha = 1.
  relerr   per element, the first-order bound of |x_dev - x| / x in units of u = 2^-53 when the device's log, sqrt, cospi
           and pow are within LIB_ULP of the true value and everything else is rounded once (see `draws`).
and `box_distance` the distance of every draw to the nearest bound, relative to the component."""
import numpy as np

U = 2.0 ** -53
M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
NORMAL, ACCEPT, OWN = 0, 1, 2
MAX_ATTEMPTS = 64
LIB_ULP = 2.0   # assumed error of a library function, in ulp of its result


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds on uint64 arrays holding 32-bit words -> the four output words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2     # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniform_pair(w0, w1, w2, w3):
    a = ((w0 << np.uint64(32)) | w1) >> np.uint64(11)
    b = ((w2 << np.uint64(32)) | w3) >> np.uint64(11)
    return (a.astype(np.float64) + 0.5) * U, (b.astype(np.float64) + 0.5) * U


def uniforms(t, j, attempt, purpose, seed):
    """U(t, j, a, p): counter (t mod 2^32, t >> 32, j + 65536 p, a), key (seed mod 2^32, seed >> 32)"""
    t = np.asarray(t, dtype=np.uint64)
    seed = int(seed)
    z = np.zeros_like(t)
    return uniform_pair(*philox4x32_10(t & M32, t >> np.uint64(32), z + np.uint64(j + 65536 * purpose), z + np.uint64(attempt),
                                       seed & 0xFFFFFFFF, seed >> 32))


def cospi(x):
    """cos(pi x) for 0 < x < 2 with the argument reduced exactly, so that the zeros keep relative accuracy"""
    y = np.where(x > 1.0, 2.0 - x, x)                     # exact; y in [0, 1]
    near0, near1 = y < 0.25, y > 0.75
    mid = ~(near0 | near1)
    out = np.empty_like(y)
    out[near0] = np.cos(np.pi * y[near0])
    out[near1] = -np.cos(np.pi * (1.0 - y[near1]))
    out[mid] = np.sin(np.pi * (0.5 - y[mid]))
    return out


def box_muller(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * cospi(2.0 * u2)


def component(alpha):
    """-> (method, D, C, 1 / alpha): 'exp' for alpha = 1, 'mt' above, 'boost' below"""
    alpha = float(alpha)
    if alpha == 1.0:
        return "exp", 0.0, 0.0, 1.0
    a = alpha if alpha > 1.0 else alpha + 1.0
    D = a - 1.0 / 3.0
    return ("mt" if alpha > 1.0 else "boost"), D, 1.0 / np.sqrt(9.0 * D), 1.0 / alpha


def gamma(t, j, alpha, seed):
    """g_j of the draws t -> (g, margin, relerr in u)"""
    t = np.asarray(t, dtype=np.uint64)
    method, D, C, inv_alpha = component(alpha)
    if method == "exp":
        u1, _ = uniforms(t, j, 0, OWN, seed)
        return -np.log(u1), np.full(t.shape, np.inf), np.full(t.shape, LIB_ULP)
    g = np.full(t.shape, D)
    margin = np.full(t.shape, np.inf)
    rel = np.zeros(t.shape)
    todo = np.ones(t.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(MAX_ATTEMPTS):
            idx = np.nonzero(todo)[0]
            if idx.size == 0:
                break
            u1, u2 = uniforms(t[idx], j, a, NORMAL, seed)
            z = box_muller(u1, u2)
            w = 1.0 + C * z
            pos = w > 0.0
            v = (w * w) * w
            q, _ = uniforms(t[idx], j, a, ACCEPT, seed)
            z2 = z * z
            squeeze = q < 1.0 - 0.0331 * (z2 * z2)
            gap = (0.5 * z2 + D * ((1.0 - v) + np.log(np.where(pos, v, 1.0)))) - np.log(q)
            acc = pos & (squeeze | (gap > 0.0))
            margin[idx] = np.minimum(margin[idx], np.where(pos, np.minimum(np.abs(w), np.abs(gap)), np.abs(w)))
            hit = idx[acc]
            g[hit] = D * v[acc]
            # z: log LIB, sqrt halves it and adds LIB, cospi LIB, the product 1/2; C z another 1/2; w = 1 + C z keeps the
            # absolute error of C z and adds 1/2; the cube triples; D v adds 1/2 + 1/2
            z_err = 0.5 * LIB_ULP + LIB_ULP + LIB_ULP + 1.0
            rel[hit] = 3.0 * (z_err * np.abs(w[acc] - 1.0) / w[acc] + 0.5) + 1.5
            todo[hit] = False
    if method == "boost":
        u1, _ = uniforms(t, j, 0, OWN, seed)
        g = g * np.power(u1, inv_alpha)
        rel = rel + LIB_ULP + 0.5
    return g, margin, rel


def draws(first, n, alphas, c_scale=1.0, seed=0, full=False):
    """rows [first, first + n) of the stream -> x (n, d); with full=True also (margin (n,), relerr (n, d)).
    relerr: x_j = (c g_j) / S has the error of g_j, of S -- the g_i weighted by g_i / S, plus (d - 1) / 2 for the additions --
    and 1 for the product and the quotient."""
    alphas = np.asarray(alphas, dtype=np.float64)
    t = np.uint64(first) + np.arange(n, dtype=np.uint64)
    cols = [gamma(t, j, alphas[j], seed) for j in range(alphas.shape[0])]
    g = [c[0] for c in cols]
    s = g[0].copy()
    for gj in g[1:]:
        s = s + gj
    x = np.stack([(c_scale * gj) / s for gj in g], axis=1)
    if not full:
        return x
    margin = np.min(np.stack([c[1] for c in cols], axis=1), axis=1)
    rel_g = np.stack([c[2] for c in cols], axis=1)
    rel_s = np.sum(rel_g * (np.stack(g, axis=1) / s[:, None]), axis=1) + 0.5 * (alphas.shape[0] - 1)
    return x, margin, rel_g + rel_s[:, None] + 1.0


def in_box(x, bounds):
    bounds = np.asarray(bounds, dtype=np.float64)
    return np.all((bounds[None, :, 0] <= x) & (x <= bounds[None, :, 1]), axis=1)


def box_distance(x, bounds):
    """per draw, the smallest |x_j - bound| / x_j.  Relative to x_j because the error of x_j is: device and restatement can put
    x_j on different sides of a bound only if it lies within a few hundred u x_j of it.  (An absolute distance would count every
    small x_j as close to a lower bound of 0, which no positive x_j can cross: with alpha_j = 0.3 one draw in 500 is below 1e-9.)"""
    bounds = np.asarray(bounds, dtype=np.float64)
    return np.min(np.minimum(np.abs(x - bounds[None, :, 0]), np.abs(x - bounds[None, :, 1])) / x, axis=1)


def sample(bounds, n_samples, alphas, c_scale=1.0, seed=0, max_zshots=500, chunk_size=1_000_000, full=False):
    """The shot and stop rule: shot s holds the draws [s chunk, (s + 1) chunk); the result is the first n_samples accepted draws
    in increasing index, zeros after them; n_drawn = chunk times the shots that were needed.
    -> (samples, n_found, n_drawn, indices of the accepted draws); with full=True also the smallest margin, the smallest
    distance to a bound and the relerr rows of the accepted draws, over the shots examined."""
    d = np.asarray(alphas).shape[0]
    out = np.zeros((n_samples, d))
    rel = np.zeros((n_samples, d))
    idx = np.zeros(n_samples, dtype=np.int64)
    found, shots = 0, 0
    margin, dist = np.inf, np.inf
    while shots < max_zshots and found < n_samples:
        x, m, r = draws(shots * chunk_size, chunk_size, alphas, c_scale, seed, full=True)
        ok = np.nonzero(in_box(x, bounds))[0]
        margin, dist = min(margin, float(m.min())), min(dist, float(box_distance(x, bounds).min()))
        take = ok[: n_samples - found]
        out[found: found + take.size] = x[take]
        rel[found: found + take.size] = r[take]
        idx[found: found + take.size] = shots * chunk_size + take
        found += take.size
        shots += 1
    res = (out, found, shots * chunk_size, idx[:found])
    return res + (margin, dist, rel) if full else res
