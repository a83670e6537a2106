"""Float64 oracle, a-priori rounding bounds and an element-wise checker for the fused eval_sh (include/wg_sh_eval.h,
csrc/sh_eval.hip), with a float32 NumPy emulation of the kernels' arithmetic and the inputs the edge tests share
(tests/test_sh_eval_edges.py).  NumPy only: importable without torch and without a device.

The oracle states the reference's real-SH polynomials (wildgaussians/method.py:493-548, constants :462-479) as a table of monomials:
values, derivatives (the power rule on each monomial, x, y, z independent as wg_sh_eval.h specifies) and the absolute-monomial
values the bounds need all come from that one table -- a different restatement from the factored expressions of the kernel and of
tests/test_sh_eval.py, so that the two check each other.

Bounds (u = 2^-24, N = (deg + 1)^2; |B|_k is basis polynomial k with every coefficient and every one of x, y, z replaced by its
absolute value and every subtraction by an addition):

  out[p, c]         (N + 8) u sum_{k<N} |sh[p, c, k]| |B|_k
                    N - 1 accumulations, 1 product, at most 7 roundings on any chain inside a basis value (k = 12, the 3xx term:
                    xx, 3 xx, two subtractions, the float32 constant, constant * z, * the bracket)
  grad_sh[p, c, k]  8 u |cot[p, c]| |B|_k for k < N; exactly 0 for k >= N
  grad_dirs[p, i]   R u sum_{k<N} S_k |dB_k / d x_i|,  S_k = sum_c |cot[p, c]| |sh[p, c, k]|,  R = 16 (GRAD_DIRS_ROUNDINGS below)

each plus N_OPS * 2^-126, so that neither gradual underflow nor flush-to-zero matters.  A fused multiply-add rounds once where the
separate operations round twice, so the bounds hold whether or not the compiler contracts.
"""
import collections

import numpy as np

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]

U = 2.0 ** -24
TINY = 2.0 ** -126
N_OPS = 128   # more than the float operations that feed any one output element at degree 3 (6 products of x, y, z, 16 basis values of
#               at most 8 operations, 16 products and sums a channel, the 40 monomials of the direction's gradient)

# The longest chain of roundings from the inputs to a component of grad_dirs, in sh_dir_grad of csrc/sh_eval.hip at degree 3 -- the
# s9 * (3 xx - 3 yy) term of gy:
#   3  s_9 = sum_c cot[c] sh[c][9]: one product (the sum starts at an exact 0), two additions
#   2  the float32 constant C3[0], and C3[0] * s_9
#   4  xx, 3 xx, the subtraction, the product with s9
#   6  the six additions that follow it in the expression (it is the first of seven terms)
#   1  gy += the expression
# = 16.  Every other chain is shorter: s9 * 6 * xy of gx has 3 + 2 + 3 + 6 + 1 = 15, s11 * (4 zz - xx - 3 yy) of gy 3 + 2 + 4 + 5 + 1 = 15,
# s12 * (6 zz - 3 xx - 3 yy) of gz 3 + 2 + 5 + 3 + 1 = 14, the degree-2 terms at most 3 + 2 + 1 + 3 + 2 = 11, the degree-1 terms 3 + 2 + 2 = 7.
GRAD_DIRS_ROUNDINGS = 16

# basis k = CONST[k] * sum of (factor, power of x, power of y, power of z)
CONST = [C0, -C1, C1, -C1] + C2 + C3
MONOMIALS = [
    [(1, 0, 0, 0)],
    [(1, 0, 1, 0)],
    [(1, 0, 0, 1)],
    [(1, 1, 0, 0)],
    [(1, 1, 1, 0)],
    [(1, 0, 1, 1)],
    [(2, 0, 0, 2), (-1, 2, 0, 0), (-1, 0, 2, 0)],
    [(1, 1, 0, 1)],
    [(1, 2, 0, 0), (-1, 0, 2, 0)],
    [(3, 2, 1, 0), (-1, 0, 3, 0)],
    [(1, 1, 1, 1)],
    [(4, 0, 1, 2), (-1, 2, 1, 0), (-1, 0, 3, 0)],
    [(2, 0, 0, 3), (-3, 2, 0, 1), (-3, 0, 2, 1)],
    [(4, 1, 0, 2), (-1, 3, 0, 0), (-1, 1, 2, 0)],
    [(1, 2, 0, 1), (-1, 0, 2, 1)],
    [(1, 3, 0, 0), (-3, 1, 2, 0)],
]
TENSORS = ("out", "grad_sh", "grad_dirs")


def n_coefficients(deg):
    return (deg + 1) ** 2


def _derivative(monomials, axis):
    """The power rule on each monomial; a monomial that does not hold the variable has no derivative term at all."""
    out = []
    for m in monomials:
        e = list(m[1:])
        if e[axis] == 0:
            continue
        f = m[0] * e[axis]
        e[axis] -= 1
        out.append((f, *e))
    return out


def _polynomial(monomials, d, absolute=False):
    """sum of factor * x^a y^b z^c over [P, 3] float64 directions (0^0 = 1); `absolute`: |factor| |x|^a |y|^b |z|^c."""
    if absolute:
        d = np.abs(d)
    v = np.zeros(d.shape[0])
    for f, a, b, c in monomials:
        v = v + (abs(f) if absolute else f) * d[:, 0] ** a * d[:, 1] ** b * d[:, 2] ** c
    return v


def _widen(sh, dirs, cot):
    for t in (sh, dirs, cot):
        assert t.dtype == np.float32, "the oracle takes the kernel's own float32 inputs"
    return sh.astype(np.float64), dirs.astype(np.float64), cot.astype(np.float64)


def oracle(deg, sh, dirs, cot):
    """out [P, 3], grad_sh [P, 3, K], grad_dirs [P, 3] in float64 from the float32 inputs widened to float64."""
    n = n_coefficients(deg)
    sh, dirs, cot = _widen(sh, dirs, cot)
    P, K = sh.shape[0], sh.shape[2]
    assert sh.shape == (P, 3, K) and dirs.shape == (P, 3) and cot.shape == (P, 3) and K >= n
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.zeros((P, 3))
        grad_sh = np.zeros((P, 3, K))
        grad_dirs = np.zeros((P, 3))
        for k in range(n):
            basis = CONST[k] * _polynomial(MONOMIALS[k], dirs)
            out = out + sh[:, :, k] * basis[:, None]
            grad_sh[:, :, k] = cot * basis[:, None]
            s = (cot * sh[:, :, k]).sum(axis=1)
            for axis in range(3):
                dm = _derivative(MONOMIALS[k], axis)
                if dm:
                    grad_dirs[:, axis] = grad_dirs[:, axis] + s * (CONST[k] * _polynomial(dm, dirs))
    return {"out": out, "grad_sh": grad_sh, "grad_dirs": grad_dirs}


def bounds(deg, sh, dirs, cot):
    """Per-element float64 bounds on |kernel - oracle| (module docstring).  grad_sh is bounded by 0 for k >= N."""
    n = n_coefficients(deg)
    sh, dirs, cot = _widen(sh, dirs, cot)
    P, K = sh.shape[0], sh.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.zeros((P, 3))
        b_sh = np.zeros((P, 3, K))
        g = np.zeros((P, 3))
        for k in range(n):
            basis = abs(CONST[k]) * _polynomial(MONOMIALS[k], dirs, absolute=True)
            a = a + np.abs(sh[:, :, k]) * basis[:, None]
            b_sh[:, :, k] = 8 * U * np.abs(cot) * basis[:, None] + N_OPS * TINY
            s = (np.abs(cot) * np.abs(sh[:, :, k])).sum(axis=1)
            for axis in range(3):
                dm = _derivative(MONOMIALS[k], axis)
                if dm:
                    g[:, axis] = g[:, axis] + s * (abs(CONST[k]) * _polynomial(dm, dirs, absolute=True))
    return {"out": (n + 8) * U * a + N_OPS * TINY, "grad_sh": b_sh, "grad_dirs": GRAD_DIRS_ROUNDINGS * U * g + N_OPS * TINY}


def check(got, deg, sh, dirs, cot, ref=None, bound=None):
    """Assert every element of every tensor in `got` (any of out, grad_sh, grad_dirs) against the oracle within its bound, and return
    {tensor: largest error / bound}.  No element is left out: where the oracle is NaN (a NaN input reaches that element) the kernel
    must give NaN, everywhere else a finite value within the bound; where the bound is 0 the value must be exactly 0."""
    ref = oracle(deg, sh, dirs, cot) if ref is None else ref
    bound = bounds(deg, sh, dirs, cot) if bound is None else bound
    ratios, failures = {}, []
    for name in TENSORS:
        if name not in got:
            continue
        g, r, b = np.asarray(got[name], dtype=np.float64), ref[name], bound[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if g.size == 0:
            ratios[name] = 0.0
            continue
        nan = np.isnan(r)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(g - r)
            ratio = np.where(err == 0, 0.0, err / np.where(nan, 1.0, b))   # a non-zero error over a zero bound is inf
        ratio = np.where(nan, np.where(np.isnan(g), 0.0, np.inf), np.where(np.isnan(ratio), np.inf, ratio))
        ratios[name] = float(ratio.max())
        if not ratios[name] <= 1.0:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            failures.append(f"{name}{list(map(int, i))}: got {g[i]!r}, oracle {r[i]!r}, bound {b[i]!r} (error / bound {ratio[i]:.3g}; "
                            f"{int((ratio > 1).sum())} of {ratio.size} elements over)")
    assert not failures, "; ".join(failures)
    return ratios


# ---- a float32 emulation of the four kernels' arithmetic (csrc/sh_eval.hip), operation for operation ---------------------------------
F32 = np.float32


class _Arithmetic:
    """float32 operations on arrays; `fused`: a * b + c keeps the product in float64 before the add (standing in for an FMA)."""

    def __init__(self, fused):
        self.fused = fused

    @staticmethod
    def mul(a, b):
        return np.multiply(a, b, dtype=F32)

    @staticmethod
    def add(a, b):
        return np.add(a, b, dtype=F32)

    @staticmethod
    def sub(a, b):
        return np.subtract(a, b, dtype=F32)

    def fma(self, a, b, c):
        if self.fused:
            return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)
        return self.add(self.mul(a, b), c)


MUTANTS = ("sign", "c3_1", "drop_s14", "k_equals_n", "tail_row", "stale_grad_sh", "swap_rows")


def _emulated_basis(deg, x, y, z, ar, c3):
    """sh_basis<DEG>: the factored expressions in the kernel's order of operations."""
    f = F32
    b = [np.full_like(x, f(C0))]
    if deg > 0:
        b += [ar.mul(f(-C1), y), ar.mul(f(C1), z), ar.mul(f(-C1), x)]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = ar.mul(x, x), ar.mul(y, y), ar.mul(z, z), ar.mul(x, y), ar.mul(y, z), ar.mul(x, z)
        b += [ar.mul(f(C2[0]), xy), ar.mul(f(C2[1]), yz), ar.mul(f(C2[2]), ar.sub(ar.fma(f(2), zz, -xx), yy)), ar.mul(f(C2[3]), xz),
              ar.mul(f(C2[4]), ar.sub(xx, yy))]
    if deg > 2:
        b += [ar.mul(ar.mul(c3[0], y), ar.fma(f(3), xx, -yy)),
              ar.mul(ar.mul(c3[1], xy), z),
              ar.mul(ar.mul(c3[2], y), ar.sub(ar.fma(f(4), zz, -xx), yy)),
              ar.mul(ar.mul(c3[3], z), ar.fma(f(-3), yy, ar.fma(f(-3), xx, ar.mul(f(2), zz)))),
              ar.mul(ar.mul(c3[4], x), ar.sub(ar.fma(f(4), zz, -xx), yy)),
              ar.mul(ar.mul(c3[5], z), ar.sub(xx, yy)),
              ar.mul(ar.mul(c3[6], x), ar.fma(f(-3), yy, xx))]
    return b


def _emulated_dir_grad(deg, x, y, z, s, ar, c3, drop_s14):
    """sh_dir_grad<DEG>: the hand-differentiated monomials in the kernel's order of operations."""
    f = F32
    gx, gy, gz = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    if deg > 0:
        gy = ar.fma(f(-C1), s[1], gy)
        gz = ar.fma(f(C1), s[2], gz)
        gx = ar.fma(f(-C1), s[3], gx)
    if deg > 1:
        s4, s5, s6, s7, s8 = (ar.mul(f(C2[i]), s[4 + i]) for i in range(5))
        s6x2, s8x2 = ar.mul(f(2), s6), ar.mul(f(2), s8)
        gx = ar.add(gx, ar.fma(s8x2, x, ar.fma(s7, z, ar.fma(-s6x2, x, ar.mul(s4, y)))))
        gy = ar.add(gy, ar.fma(-s8x2, y, ar.fma(-s6x2, y, ar.fma(s5, z, ar.mul(s4, x)))))
        gz = ar.add(gz, ar.fma(s7, x, ar.fma(ar.mul(f(4), s6), z, ar.mul(s5, y))))
    if deg > 2:
        xx, yy, zz, xy, yz, xz = ar.mul(x, x), ar.mul(y, y), ar.mul(z, z), ar.mul(x, y), ar.mul(y, z), ar.mul(x, z)
        s9, s10, s11, s12, s13, s14, s15 = (ar.mul(c3[i], s[9 + i]) for i in range(7))
        xx3_yy3 = ar.fma(f(3), xx, -ar.mul(f(3), yy))
        t = ar.mul(ar.mul(s9, f(6)), xy)
        t = ar.fma(s10, yz, t)
        t = ar.fma(-ar.mul(s11, f(2)), xy, t)
        t = ar.fma(-ar.mul(s12, f(6)), xz, t)
        t = ar.fma(s13, ar.sub(ar.fma(f(-3), xx, ar.mul(f(4), zz)), yy), t)
        if not drop_s14:
            t = ar.fma(ar.mul(s14, f(2)), xz, t)
        t = ar.fma(s15, xx3_yy3, t)
        gx = ar.add(gx, t)
        t = ar.mul(s9, xx3_yy3)
        t = ar.fma(s10, xz, t)
        t = ar.fma(s11, ar.fma(f(-3), yy, ar.sub(ar.mul(f(4), zz), xx)), t)
        t = ar.fma(-ar.mul(s12, f(6)), yz, t)
        t = ar.fma(-ar.mul(s13, f(2)), xy, t)
        t = ar.fma(-ar.mul(s14, f(2)), yz, t)
        t = ar.fma(-ar.mul(s15, f(6)), xy, t)
        gy = ar.add(gy, t)
        t = ar.mul(s10, xy)
        t = ar.fma(ar.mul(s11, f(8)), yz, t)
        t = ar.fma(s12, ar.fma(f(-3), yy, ar.fma(f(-3), xx, ar.mul(f(6), zz))), t)
        t = ar.fma(ar.mul(s13, f(8)), xz, t)
        t = ar.fma(s14, ar.sub(xx, yy), t)
        gz = ar.add(gz, t)
    return gx, gy, gz


def emulate(deg, sh, dirs, cot, fused=False, want_dirs=True, mutant=None, seed=0):
    """What the kernels compute, in float32 NumPy: every output starts as NaN (the edge tests' pre-fill) and is written wave by wave
    (64 rows), as the kernels write it.  `fused` contracts every a * b + c.  `mutant` (one of MUTANTS, placed by `seed`) plants one
    fault; the mutants exist here only, never in a kernel."""
    assert mutant is None or mutant in MUTANTS
    n = n_coefficients(deg)
    P, K = sh.shape[0], sh.shape[2]
    ar = _Arithmetic(fused)
    rng = np.random.default_rng(seed)
    c3 = [F32(c) for c in C3]
    if mutant == "c3_1":
        c3[1] = F32(C3[1] * (1 + 1e-5))
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = (np.ascontiguousarray(dirs[:, i]) for i in range(3))
        n_sum = n
        if mutant == "k_equals_n" and deg < 3 and K > n:
            n_sum = n + 1
            b = _emulated_basis(deg + 1, x, y, z, ar, c3)[:n_sum]
        else:
            b = _emulated_basis(deg, x, y, z, ar, c3)
        if mutant == "sign" and n > 1:
            k = int(rng.integers(1, n))
            b[k] = -b[k]
        out = np.empty((P, 3), F32)
        grad_sh = np.zeros((P, 3, K), F32)
        s = [np.zeros(P, F32) for _ in range(n)]
        for c in range(3):
            r = ar.mul(b[0], sh[:, c, 0])
            for k in range(1, n_sum):
                r = ar.fma(b[k], sh[:, c, k], r)
            out[:, c] = r
            for k in range(n):
                grad_sh[:, c, k] = ar.mul(b[k], cot[:, c])
                s[k] = ar.fma(cot[:, c], sh[:, c, k], s[k])
        if mutant == "stale_grad_sh":
            grad_sh[:, :, n:] = np.nan
        grad_dirs = np.stack(_emulated_dir_grad(deg, x, y, z, s, ar, c3, mutant == "drop_s14"), axis=1) if want_dirs else None
    written = {"out": np.full((P, 3), np.nan, F32), "grad_sh": np.full((P, 3, K), np.nan, F32)}
    computed = {"out": out, "grad_sh": grad_sh}
    if want_dirs:
        written["grad_dirs"], computed["grad_dirs"] = np.full((P, 3), np.nan, F32), grad_dirs
    for first in range(0, P, 64):
        valid = min(64, P - first)
        rows = np.arange(first, first + valid)
        src = rows.copy()
        if mutant == "swap_rows" and valid > 1:
            p = int(rng.integers(0, valid - 1))
            src[p], src[p + 1] = rows[p + 1], rows[p]
        if mutant == "tail_row" and valid < 64:
            rows, src = rows[:-1], src[:-1]
        for name in written:
            written[name][rows] = computed[name][src]
    return written


# ---- the inputs the edge tests share -------------------------------------------------------------------------------------------------
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def directions(P, seed):
    """Mixed within one launch, by row: unit vectors, the six axis vectors, the zero vector, unit vectors scaled by 1e-3 and by 30, and
    vectors whose components have magnitudes from 1e-3 to 10 each."""
    rng = np.random.default_rng([seed, 1])
    v = rng.normal(size=(P, 3))
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    i = np.arange(P)
    kind = (i + seed) % 8
    d[kind == 2] = AXES[(i[kind == 2] // 8 + seed) % 6]
    d[kind == 3] = 0.0
    d[kind == 4] *= 1e-3
    d[kind == 5] *= 30.0
    d[kind == 7] = (v * 10.0 ** rng.uniform(-3, 1, size=(P, 3)))[kind == 7]
    return d.astype(np.float32)


def coefficients(P, K, seed):
    return np.random.default_rng([seed, 2]).normal(size=(P, 3, K)).astype(np.float32)


def cotangent(P, seed, zero_channel=None):
    """Normal, a seventh of the elements exactly 0; `zero_channel`: that channel 0 throughout."""
    rng = np.random.default_rng([seed, 3])
    g = rng.normal(size=(P, 3))
    g[rng.random(size=(P, 3)) < 1 / 7] = 0.0
    if zero_channel is not None:
        g[:, zero_channel] = 0.0
    return g.astype(np.float32)


def one_hot(K=16, rows=192):
    """Row r has a single non-zero coefficient, at channel r % 3 and k = (r // 3) % 16."""
    sh = np.zeros((rows, 3, K), np.float32)
    r = np.arange(rows)
    sh[r, r % 3, (r // 3) % 16] = np.random.default_rng([0, 4]).uniform(0.5, 2.0, size=rows) * np.where(r % 2, -1.0, 1.0)
    return sh


# P, degree, K, which pointer sits 4 bytes off a 16-byte boundary (None, "sh", or "grad_sh": the latter in the backward only)
Case = collections.namedtuple("Case", "P deg K misalign")
WAVE_EDGES = (1, 63, 64, 65, 191, 256, 257, 320)   # 320: the second block has one full wave and three empty ones
CASES = (
    # K = 16, every pointer 16-byte aligned: the k16 kernels
    [Case(P, 3, 16, None) for P in WAVE_EDGES] + [Case(P, deg, 16, None) for deg in (0, 1, 2) for P in (65, 320)]
    # K = 16, a pointer 4 bytes off: the generic kernels with vec = false
    + [Case(257, deg, 16, "sh") for deg in (0, 1, 2, 3)] + [Case(63, 3, 16, "sh")]
    + [Case(257, 1, 16, "grad_sh"), Case(257, 3, 16, "grad_sh"), Case(65, 2, 16, "grad_sh")]
    # K in {20, 12, 4}: the generic kernels' 16-byte path (the run-time quad loop, the zero fill when K > N)
    + [Case(257, deg, 20, None) for deg in (0, 1, 2, 3)] + [Case(65, 3, 20, None)]
    + [Case(191, deg, 12, None) for deg in (0, 1, 2)] + [Case(65, deg, 4, None) for deg in (0, 1)]
    # K in {9, 25, 1}: the scalar path
    + [Case(257, deg, 9, None) for deg in (0, 1, 2)] + [Case(191, deg, 25, None) for deg in (0, 1, 2, 3)]
    + [Case(65, 0, 1, None), Case(1, 0, 1, None)]
)


def case_id(c):
    return f"P{c.P}-deg{c.deg}-K{c.K}" + (f"-{c.misalign}+4B" if c.misalign else "")


def kernel_path(c, backward=False):
    """Which kernel the dispatch rules of csrc/sh_eval.hip send the case to, and with which run-time `vec` flag.  (With `vec` set the
    generic forward still loads scalars where N % 4 != 0, degrees 0 and 2; the backward's 16-byte stores depend on `vec` alone.)"""
    off = c.misalign == "sh" or (backward and c.misalign == "grad_sh")
    if c.K == 16 and not off:
        return "k16"
    return "generic_vec16" if c.K % 4 == 0 and not off else "generic_scalar"


def case_inputs(c):
    """sh, dirs, cot of a case.  The cotangent's all-zero channel moves with the case (none for a quarter of them)."""
    seed = CASES.index(c)
    zc = seed % 4
    return coefficients(c.P, c.K, seed), directions(c.P, seed), cotangent(c.P, seed, zc if zc < 3 else None)


def one_hot_inputs():
    return one_hot(), directions(192, 5), cotangent(192, 5)
