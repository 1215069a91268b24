"""tf.train.AdamOptimizer restated for the tests of csrc/adam.hip (hmmr_adam_step) and human_dynamics_amd/optim.py.

`step32` is the oracle the kernel is held to BYTE FOR BYTE: the published TF 1.x ApplyAdam functor, operation by operation on float32
NumPy arrays (every NumPy operation on float32 operands rounds once to float32; sqrt and the division are correctly rounded; nothing
is fused) --
    on the host:  alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power)
    per element:  m += (g - m) * (1 - beta1);   v += (g * g - v) * (1 - beta2);   p -= (m * alpha) / (sqrt(v) + eps)
with the beta powers float32 values multiplied by beta after each step (AdamOptimizer._finish).

`closed64` is the same optimiser in its closed form in float64 (m_t and v_t as sums; the bias correction from TF's float32 power products): test_adam_cases.py holds
the oracle to it within a few float32 units over 12 steps, and separates both from torch.optim.Adam's form (epsilon added AFTER the
bias correction of v), so the oracle cannot silently be the wrong Adam.

The GPU cases (test_gpu_adam.py): segment lengths around the 16-byte piece, the wave and the kernel's chunk of 4096 values, every
placement of the four pointers at float offsets 0 .. 3, and gradients whose every intermediate stays a normal float32 or an exact zero
(denormal behaviour is not asserted)."""
import numpy as np

F = np.float32
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 1023, 4097)
OFFSETS = (0, 1, 2, 3)
SEGMENT_COUNTS = (1, 2, 64, 65)
CHECK_STEPS = (1, 2, 3, 12)
GUARD = 0x7FC12345            # a quiet NaN with a payload: the bit pattern of every float no kernel may touch
GUARD_FLOATS = 8


def powers(beta, k):
    """the beta power TF holds BEFORE step k + 1 (k = 0: beta itself), as a float32 product"""
    p = F(beta)
    for _ in range(k):
        p = F(p * F(beta))
    return p


def alpha32(lr, beta1_power, beta2_power):
    return F(F(lr) * np.sqrt(F(1) - F(beta2_power)) / (F(1) - F(beta1_power)))


def step32(p, g, m, v, beta1_power, beta2_power, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """one ApplyAdam on float32 arrays -> (p, m, v), new arrays"""
    p, g, m, v = (np.asarray(x, F) for x in (p, g, m, v))
    alpha = alpha32(lr, beta1_power, beta2_power)
    m = m + (g - m) * (F(1) - F(beta1))
    v = v + (g * g - v) * (F(1) - F(beta2))
    p = p - (m * alpha) / (np.sqrt(v) + F(eps))
    assert p.dtype == m.dtype == v.dtype == F
    return p, m, v


def run32(p, grads, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """[(p, m, v) after step 1, 2, ...] for a list of gradients, moments from zero"""
    p = np.asarray(p, F)
    m, v, out = np.zeros_like(p), np.zeros_like(p), []
    for k, g in enumerate(grads):
        p, m, v = step32(p, g, m, v, powers(beta1, k), powers(beta2, k), lr, beta1, beta2, eps)
        out.append((p, m, v))
    return out


def closed64(p, grads, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """the same steps in float64 from the closed forms m_t = (1 - b1) sum_i b1^(t-i) g_i, v_t likewise.  The bias correction takes TF's
    float32 power products (`powers`): they are part of what TF computes, not a rounding of it -- 1 - beta2_power is ~0.001 t, so the
    6e-8 steps of a float32 near 1 move alpha by up to 3e-5 / t relative, a hundred float32 units of a step, against beta2 ** t."""
    lr, beta1, beta2, eps = (float(F(x)) for x in (lr, beta1, beta2, eps))          # the hyper-parameters ARE float32 values
    p = np.asarray(p, np.float64).copy()
    gs, out = [np.asarray(g, np.float64) for g in grads], []
    for t in range(1, len(gs) + 1):
        m = (1 - beta1) * sum(beta1 ** (t - i) * gs[i - 1] for i in range(1, t + 1))
        v = (1 - beta2) * sum(beta2 ** (t - i) * gs[i - 1] ** 2 for i in range(1, t + 1))
        p = p - lr * np.sqrt(1 - float(powers(beta2, t - 1))) / (1 - float(powers(beta1, t - 1))) * m / (np.sqrt(v) + eps)
        out.append((p.copy(), m, v))
    return out


def torch_form64(p, grads, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """torch.optim.Adam's form in float64: p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)"""
    lr, beta1, beta2, eps = (float(F(x)) for x in (lr, beta1, beta2, eps))
    p = np.asarray(p, np.float64).copy()
    m, v, out = np.zeros_like(p), np.zeros_like(p), []
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, np.float64)
        m = beta1 * m + (1 - beta1) * g
        v = beta2 * v + (1 - beta2) * g * g
        p = p - lr / (1 - beta1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps)
        out.append(p.copy())
    return out


def gradients(kind, n, step, seed=0):
    """float32 gradients of a segment: 'mixed' magnitudes 1e-12 .. 1e2 with both signs, 'zeros', 'some_zeros' (mixed with a third of
    the values exactly 0).  |g| >= 1e-12 keeps g * g * (1 - beta2) >= 1e-27 and m * alpha >= 1e-17: every intermediate is normal."""
    rng = np.random.default_rng([seed, n, step, len(kind)])
    if kind == "zeros":
        return np.zeros(n, F)
    g = (10.0 ** rng.uniform(-12, 2, n) * rng.choice((-1.0, 1.0), n)).astype(F)
    if kind == "some_zeros":
        g[rng.random(n) < 1 / 3] = 0
    return g


def values(n, seed):
    return np.random.default_rng([seed, n, 99]).standard_normal(n).astype(F)


def ulps32(a, b):
    """|a - b| in units of the float32 spacing at b"""
    b = np.asarray(b, np.float64)
    return np.abs(np.asarray(a, np.float64) - b) / np.spacing(np.abs(b).astype(F)).astype(np.float64)


# every refusal of hmmr_adam_step: (name, changes to a good call, words of the message)
ADAM_REFUSALS = (
    ("null hyper", dict(h=None), "null hyper-parameters"),
    ("negative count", dict(n_segs=-1), "-1 segments"),
    ("null table", dict(segs=None), "null table"),
    ("lr nan", dict(lr=float("nan")), "lr is not finite"),
    ("beta1 inf", dict(beta1=float("inf")), "beta1 is not finite"),
    ("beta2 nan", dict(beta2=float("nan")), "beta2 is not finite"),
    ("eps inf", dict(eps=float("-inf")), "eps is not finite"),
    ("beta1_power nan", dict(beta1_power=float("nan")), "beta1_power is not finite"),
    ("beta2_power inf", dict(beta2_power=float("inf")), "beta2_power is not finite"),
    ("beta1_power 0", dict(beta1_power=0.0), "beta1_power=0 lies outside (0, 1)"),
    ("beta1_power 1", dict(beta1_power=1.0), "beta1_power=1 lies outside (0, 1)"),
    ("beta2_power 1", dict(beta2_power=1.0), "beta2_power=1 lies outside (0, 1)"),
    ("beta2_power negative", dict(beta2_power=-0.5), "beta2_power=-0.5 lies outside (0, 1)"),
    ("negative n", dict(n=-1), "segment 1 has n=-1"),
    ("n beyond 2^40", dict(n=(1 << 40) + 1), "segment 1 has n=1099511627777 (0 .. 2^40)"),
    ("null p", dict(p=None), "segment 1 has a null p, m or v"),
    ("null m", dict(m=None), "segment 1 has a null p, m or v"),
    ("null v", dict(v=None), "segment 1 has a null p, m or v"),
    ("null v without g", dict(v=None, g=None), "segment 1 has a null p, m or v"),
    ("misaligned g", dict(g=0x4002), "segment 1 has a pointer that is not 4-byte aligned"),
    ("misaligned p", dict(p=0x1001), "segment 1 has a pointer that is not 4-byte aligned"),
)

# ... and of hmmr_strip_mse
MSE_REFUSALS = (
    ("null a", dict(a=None), "null a or b"),
    ("null b", dict(b=None), "null a or b"),
    ("no rows", dict(rows=0), "rows=0 and cols=7 must be positive"),
    ("negative cols", dict(cols=-2), "cols=-2 must be positive"),
    ("too many rows", dict(rows=(1 << 24) + 1, ws_bytes=1 << 40), "exceed 2^24"),
    ("short lda", dict(lda=6), "lda=6 or ldb=7 is below cols=7"),
    ("short ldb", dict(ldb=0), "is below cols=7"),
    ("no output", dict(loss=None, d_a=None, d_b=None), "nothing to write"),
    ("short ld_da", dict(ld_da=6), "ld_da=6 or ld_db=7 is below cols=7"),
    ("short ld_db", dict(ld_db=3), "is below cols=7"),
    ("weight nan", dict(weight=float("nan")), "weight is not finite"),
    ("weight inf", dict(weight=float("inf")), "weight is not finite"),
    ("null workspace", dict(ws=None), "workspace too small"),
    ("small workspace", dict(ws_bytes=255), "workspace too small (255 bytes given, 256 needed)"),
)
