"""numpy restatements of the update stage (csrc/update.hip: NaN filter, per-tensor clip_by_norm, Keras Adam) and the rule the tests
hold it to.

    chunk_rule(lens, C)               the chunk table as a list of (offset, length, tensor, first chunk of the tensor, its chunks)
    chunk_partial / tensor_norms      the documented float64 order of the sum of squares, and l2 = float32(sqrt(sum)) per tensor
    twin_update(g, l2, p, m, v, ...)  the five float32 lines, one rounding per operation (the library is built with -ffp-contract=off),
                                      given l2 per element
    reference_update(...)             the whole update in float64 on the float32 operands (alpha, clip, b1, b2 and eps included)
                                      promoted to float64, its norm a plain float64 sum
    reference_update_torch_eps(...)   a WRONG formula here (negative control): torch.optim.Adam's epsilon placement, inside the bias
                                      correction, in float64
    bars(...)                         a first-order float32 error bar per element for m, v and p; u = 2^-24

The bar, per element, every term taken from the float64 reference (primes: the values after the step; omb = 1 - b, which float32
evaluates exactly for 0.5 <= b < 1, Sterbenz, and which the reference takes from the same float32 b):
    gc = (g0 clip) / max(l2, clip)     two roundings and the float32 rounding of l2:         d_gc  = 3 u |gc|
    m' = m + (gc - m) omb1             the subtraction u (|gc| + |m|), the product u |gc - m| omb1 <= u (|gc| + |m|) omb1, the sum u |m'|:
                                       d_m   = u (3 |gc| omb1 + 2 (|gc| + |m|) omb1 + |m'|)
    v' = v + (gc gc - v) omb2          gc gc carries 2 d_gc |gc| + u gc^2 = 7 u gc^2, then as m':
                                       d_v   = u (7 gc^2 omb2 + 2 (gc^2 + |v|) omb2 + |v'|)
    den = sqrt(v') + eps               d_den = d_v / (2 sqrt(v')) + u sqrt(v') + u den        (v' = 0: the first term is 0, d_v is)
    step = (m' alpha) / den            d_step = d_m alpha / den + |step| (2 u + d_den / den)
    p' = p - step                      d_p   = d_step + u |p'|
The rule: |twin - reference| <= MARGIN * bar for every element whose reference is finite, MARGIN = 2 for the second-order terms the bar
leaves out; elements whose reference is not finite must agree in kind.  The device is not held to this bar but to the twin's bits
(tests/test_gpu_update.py); the bar says that those bits are the float64 formula's to float32 precision -- and that torch's epsilon
placement is not."""
import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -24
MARGIN = 2.0
THREADS = 256            # one quad of the chunk per thread: C = 4 * THREADS


def adam_alpha(t, lr, beta1, beta2):
    """float32(lr sqrt(1 - beta2^t) / (1 - beta1^t)), every operation in float64 (restated, not imported from the package)."""
    return F(float(lr) * np.sqrt(1.0 - float(beta2) ** int(t)) / (1.0 - float(beta1) ** int(t)))


# ---- the chunk rule and the order of the sum ---------------------------------------------------------------------------------
def chunk_rule(lens, C):
    out, off, c = [], 0, 0
    for k, n in enumerate(lens):
        count = -(-int(n) // C)
        for j in range(count):
            out.append((off + j * C, min(C, int(n) - j * C), k, c, count))
        off, c = off + int(n), c + count
    return out


def chunk_partial(g, C):
    """float64 partials of the chunks of ONE tensor's float32 gradient g, in launch 1's order: per thread the quad's four squares
    ascending, per wave the xor butterfly 32 .. 1, then the waves ascending."""
    g = np.asarray(g, F).reshape(-1)
    assert C == 4 * THREADS
    count = -(-g.size // C)
    d = np.zeros(count * C, D)
    g0 = np.where(np.isnan(g), F(0), g).astype(D)
    with np.errstate(over="ignore"):
        d[:g.size] = g0 * g0
    q = d.reshape(count, THREADS, 4)
    with np.errstate(invalid="ignore"):
        s = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
        x = s.reshape(count, THREADS // 64, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            x = x + x[..., lane ^ off]
        w = x[..., 0]
        part = w[:, 0]
        for k in range(1, THREADS // 64):
            part = part + w[:, k]
    return part


def tensor_norms(flat, lens, C):
    """float32 l2 per tensor: the tensor's partials added one at a time in ascending chunk order, sqrt, one rounding to float32."""
    out, off = np.empty(len(lens), F), 0
    for k, n in enumerate(lens):
        s = D(0.0)
        for part in chunk_partial(flat[off:off + n], C):
            s = s + part
        out[k] = F(np.sqrt(s))
        off += n
    return out


# ---- the five lines ----------------------------------------------------------------------------------------------------------
def twin_update(g, l2, p, m, v, alpha, clip, b1, b2, eps):
    """(p', m', v') float32; l2 per element (a tensor's norm repeated over its elements) or a scalar."""
    g, p, m, v = (np.asarray(a, F) for a in (g, p, m, v))
    l2, alpha, clip, b1, b2, eps = np.asarray(l2, F), F(alpha), F(clip), F(b1), F(b2), F(eps)
    with np.errstate(all="ignore"):
        g0 = np.where(np.isnan(g), F(0), g)
        gc = (g0 * clip) / np.maximum(l2, clip)
        m = m + (gc - m) * (F(1) - b1)
        v = v + (gc * gc - v) * (F(1) - b2)
        p = p - (m * alpha) / (np.sqrt(v) + eps)
    assert p.dtype == F and m.dtype == F and v.dtype == F
    return p, m, v


def _ref_terms(g, lens, p, m, v, alpha, clip, b1, b2, eps):
    g, p, m, v = (np.asarray(a, F).astype(D) for a in (g, p, m, v))
    alpha, clip, b1, b2, eps = (D(F(a)) for a in (alpha, clip, b1, b2, eps))
    g0 = np.where(np.isnan(g), 0.0, g)
    l2 = np.concatenate([np.full(n, np.sqrt(np.sum(part * part))) for n, part in zip(lens, np.split(g0, np.cumsum(lens)[:-1]))])
    gc = (g0 * clip) / np.maximum(l2, clip)
    m1 = m + (gc - m) * (1.0 - b1)
    v1 = v + (gc * gc - v) * (1.0 - b2)
    return g0, gc, p, m, v, m1, v1, alpha, b1, b2, eps


def reference_update(g, lens, p, m, v, alpha, clip, b1, b2, eps):
    with np.errstate(all="ignore"):
        g0, gc, p, m, v, m1, v1, alpha, b1, b2, eps = _ref_terms(g, lens, p, m, v, alpha, clip, b1, b2, eps)
        return p - (m1 * alpha) / (np.sqrt(v1) + eps), m1, v1


def reference_update_torch_eps(g, lens, p, m, v, t, lr, clip, b1, b2, eps):
    """torch.optim.Adam's step on the same clipped gradient: p -= lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)."""
    with np.errstate(all="ignore"):
        g0, gc, p, m, v, m1, v1, _, b1, b2, eps = _ref_terms(g, lens, p, m, v, 0.0, clip, b1, b2, eps)
        return p - float(lr) / (1.0 - b1 ** t) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps), m1, v1


def bars(g, lens, p, m, v, alpha, clip, b1, b2, eps):
    """(bar_p, bar_m, bar_v), float64, per element (the derivation is in the module's docstring)."""
    with np.errstate(all="ignore"):
        g0, gc, p, m, v, m1, v1, alpha, b1, b2, eps = _ref_terms(g, lens, p, m, v, alpha, clip, b1, b2, eps)
        omb1, omb2 = 1.0 - b1, 1.0 - b2
        d_m = U * (3.0 * np.abs(gc) * omb1 + 2.0 * (np.abs(gc) + np.abs(m)) * omb1 + np.abs(m1))
        d_v = U * (7.0 * gc * gc * omb2 + 2.0 * (gc * gc + np.abs(v)) * omb2 + np.abs(v1))
        root = np.sqrt(v1)
        den = root + eps
        d_den = np.where(v1 > 0, d_v / (2.0 * np.where(v1 > 0, root, 1.0)), 0.0) + U * root + U * den
        step = (m1 * alpha) / den
        d_step = d_m * np.abs(alpha) / den + np.abs(step) * (2.0 * U + d_den / den)
        d_p = d_step + U * np.abs(p - step)
    return d_p, d_m, d_v


def worst_excess(got, want, bar):
    """(max over the elements whose reference is finite of |got - want| / bar -- an element with bar == 0 must be exact --, whether the
    other elements agree in kind: NaN with NaN, the same infinity)."""
    got, want, bar = np.asarray(got, D), np.asarray(want, D), np.asarray(bar, D)
    fin = np.isfinite(want)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        e = np.where(bar > 0, err / bar, np.where(got == want, 0.0, np.inf))
    e = np.where(np.isnan(e), np.inf, e)[fin]
    return (float(e.max()) if e.size else 0.0), bool(np.array_equal(got[~fin], want[~fin], equal_nan=True))


def same_bits(a, b):
    """Equal float32 arrays bit for bit, except that any NaN equals any NaN (non-finite values are equal in kind)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | nan))
