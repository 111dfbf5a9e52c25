"""Cases shared by tests/test_norm_edge_cases_cpu.py and tests/test_norm_edges_gpu.py: the code paths of csrc/dj_norm.hip
(BatchNormalization forward and backward, Add+ReLU, ReLU backward, strided copies, the blocked column reductions and their
finalizers, L2Normalization, max pooling, up-sampling), the inputs that reach them and plain float64 references.

No GPU is imported here.  Every tensor operand is described by a `Slab`: a rows x C view at float offset `off` with pixel
stride `ld` inside a wider buffer filled with one NaN bit pattern, so that the stride and the alignment of the base are free
parameters and everything around an output can be compared bit for bit after a launch.

Two kinds of data:
  dyadic  values k/8 with |v| <= 8, scales +-2^k, shifts and gradients k/8: every product and sum of these kernels is then
          exact in fp32 in any order (and with or without fused multiply-adds), so a result must EQUAL the float64
          reference cast to fp32.  Used wherever a mask is recomputed: no sign depends on a rounding.
  normal  random normal values, compared against float64 with the bounds derived below (U = 2^-24, half an ulp).
"""
import collections
import zlib

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
ULP = 2.0 ** -23        # one ulp, relative: a correctly rounded store of a double, or a 1-ulp rsqrtf
RB = 64                 # rows per reduction block (DJ_RB)
FIN_LANES = 64          # row lanes of the finalizers (DJ_FIN_LANES); their unrolled loop runs while r + 3*64 < nrows
FIN_CH = 16             # channels per finalizer block (DJ_FIN_CH)
COPY_PARTS = 8          # DJ_COPY_PARTS
COLSUM_PARTS = 32       # DJ_COLSUM_PARTS
SENTINEL_BITS = 0x7FC0BEEF   # a quiet NaN: a stray read poisons the result, a stray write changes the bits


# --------------------------------------------------------------------------------------------------------------------
# dispatch rules, copied from the launchers
# --------------------------------------------------------------------------------------------------------------------
def aligned16(float_off):
    """A pointer at `float_off` floats past a 16-byte aligned allocation is 16-byte aligned."""
    return float_off % 4 == 0


def v4(C, slabs, vec_offs=()):
    """The 4-wide kernel: C % 4 == 0, every ld % 4 == 0, every tensor pointer and per-channel vector 16-byte aligned."""
    return (C % 4 == 0 and all(s.ld % 4 == 0 and aligned16(s.off) for s in slabs)
            and all(aligned16(o) for o in vec_offs))


def tx_log2(C, vec4):
    """launch_colreduce: the smallest power of two of column groups >= the number of groups, within 4..64."""
    groups = C // 4 if vec4 else C
    t = 6
    while t > 2 and (1 << (t - 1)) >= groups:
        t -= 1
    return t


def column_blocks(C, vec4):
    groups = C // 4 if vec4 else C
    return -(-groups // (1 << tx_log2(C, vec4)))


def pool4(C, x_off, y_off, argmax_byte_off):
    """The 4-channel max-pool pair: C % 4 == 0, the float tensors 16-byte aligned, argmax & 3 == 0 (null counts as 0).
    `x_off`, `y_off`: float offsets of the two float tensors the launcher looks at (x, y forward; dy, dx backward)."""
    return C % 4 == 0 and aligned16(x_off) and aligned16(y_off) and (argmax_byte_off or 0) % 4 == 0


def pool_bwd_path(C, dy_off, dx_off, argmax_byte_off):
    if argmax_byte_off is None:
        return "bwd_rescan"
    return "bwd4" if pool4(C, dy_off, dx_off, argmax_byte_off) else "bwd_saved_scalar"


def fin_lane_work(nrows, lane):
    """dj_partial_sums, row lane `lane`: (iterations of the 4-rows-in-flight loop, rows left to the tail loop).  The
    unrolled loop starts at nrows > 192 for lane 0."""
    trips, r = 0, lane
    while r + 3 * FIN_LANES < nrows:
        trips, r = trips + 1, r + 4 * FIN_LANES
    return trips, len(range(r, nrows, FIN_LANES))


def fin_path(nrows):
    (t0, l0), (t1, l1) = fin_lane_work(nrows, 0), fin_lane_work(nrows, FIN_LANES - 1)
    return "fin_trips%d_%d_tail%d_%d" % (t0, t1, l0, l1)


# --------------------------------------------------------------------------------------------------------------------
# slabs
# --------------------------------------------------------------------------------------------------------------------
class Slab(object):
    """rows x C floats at buffer[off + r*ld + c] inside a sentinel-filled buffer with `tail` floats after the last row."""

    def __init__(self, rows, C, ld=None, off=0, tail=None):
        self.rows, self.C = int(rows), int(C)
        self.ld = int(C if ld is None else ld)
        self.off = int(off)
        assert self.ld >= self.C and self.off >= 0
        self.size = self.off + self.rows * self.ld + (2 * self.C + 8 if tail is None else tail)
        self.index = self.off + np.arange(self.rows)[:, None] * self.ld + np.arange(self.C)[None, :]

    def host(self, values=None):
        buf = np.full(self.size, SENTINEL_BITS, dtype=np.uint32).view(np.float32)
        if values is not None:
            buf[self.index] = np.asarray(values, dtype=np.float32).reshape(self.rows, self.C)
        return buf

    def read(self, flat):
        return np.asarray(flat).reshape(-1)[self.index]

    def surroundings_equal(self, before, after):
        keep = np.ones(self.size, dtype=bool)
        keep[self.index.reshape(-1)] = False
        return bool(np.array_equal(np.asarray(before).view(np.int32)[keep], np.asarray(after).view(np.int32)[keep]))


def vec_slab(C, off=0):
    return Slab(1, C, C, off, tail=8)


# --------------------------------------------------------------------------------------------------------------------
# path selection: one layout per reason for leaving the 4-wide kernel, and two on it
# --------------------------------------------------------------------------------------------------------------------
# C, ld of the first tensor (tensor k of a pass gets ld + 4k, so that every tensor has a stride of its own and a swapped
# stride shows), float offset and the index of the one tensor that carries it (None: all of them; -1: the last, an
# output), float offset of one per-channel vector (or of the partials where a pass has no vector), expected kernel
Layout = collections.namedtuple("Layout", "name C ld off who vec_off path")
LAYOUTS = [
    Layout("v4_dense", 8, 8, 0, None, 0, "v4"),
    Layout("v4_slice", 8, 16, 4, None, 0, "v4"),          # ld = C + 8, base offset 4
    Layout("scalar_c", 30, 32, 0, None, 0, "scalar"),     # C % 4 != 0, everything else aligned
    Layout("scalar_ld", 8, 9, 0, None, 0, "scalar"),
    Layout("scalar_off1", 8, 12, 1, 0, 0, "scalar"),
    Layout("scalar_off2", 8, 12, 2, 1, 0, "scalar"),
    Layout("scalar_off3", 8, 12, 3, -1, 0, "scalar"),
    Layout("scalar_vec", 8, 16, 4, None, 1, "scalar"),    # everything aligned except one vector
]
LAYOUT_BY_NAME = {l.name: l for l in LAYOUTS}
LAYOUT_ROWS = 65     # two row blocks of the reductions, more than one workgroup of the elementwise passes
PATH_REASONS = [l.name for l in LAYOUTS]


def layout_slabs(layout, n_tensors, rows=LAYOUT_ROWS):
    """The slabs of a pass with `n_tensors` tensor operands under `layout`."""
    who = layout.who
    if who is not None:
        who = n_tensors - 1 if who < 0 else min(who, n_tensors - 1)
    return [Slab(rows, layout.C, layout.ld + 4 * k, layout.off if who in (None, k) else 0) for k in range(n_tensors)]


# affine_act variants: name -> (scale, residual, residual affine, relu)
AFFINE_VARIANTS = collections.OrderedDict([
    ("relu_only", (False, False, False, 1)),
    ("affine", (True, False, False, 0)),
    ("affine_res_relu", (True, True, False, 1)),
    ("affine_resaffine_relu", (True, True, True, 1)),
    ("res_affine_only", (False, True, True, 0)),
])
# the scalar_vec layout moves ONE per-channel vector off 16 bytes: scale of dj_affine_act (the residual's where there is no
# scale), mean of dj_bn_bwd_reduce, k1 of dj_bn_bwd_apply; a reduction without a vector gets its partials moved instead

# column reductions
COLRED_C_V4 = [4, 12, 24, 40, 100, 260]     # tx_log2 2, 2, 3, 4, 5, 6; 260 = 65 groups: a second column block of one group
COLRED_C_SCALAR = [1, 3, 7, 30, 65]
COLRED_ROWS = [1, 63, 64, 65, 1083]
# finalizers
FIN_NROWS = [1, 63, 64, 65, 192, 193, 256, 257, 449, 704]
FIN_C = [1, 15, 16, 17, 40]
INFER_C = [1, 127, 128, 129]
COLSUM_DIRECT_ROWS = [1, 64, 193, 257]
EW_ROWS = [1, 63, 64, 65, 130]
EW_C = [1, 3, 8, 12, 30, 65, 260]
L2_C = [3, 30, 64, 65, 1024]
L2_ROWS = 13          # 4 rows per workgroup: three full workgroups and one with a single row


# --------------------------------------------------------------------------------------------------------------------
# data
# --------------------------------------------------------------------------------------------------------------------
def rng_for(*key):
    """A generator seeded by the case's own name, the same in every process."""
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def dyadic(rng, shape, lim=64):
    """Multiples of 1/8 in [-lim/8, lim/8]."""
    return (rng.integers(-lim, lim + 1, size=shape) / 8.0).astype(np.float32)


def dyadic_bn(rng, rows, C):
    """z, y, dy, scale, shift, mean, invstd, k0, k1, k2 of a BatchNormalization backward on dyadic data.  z*scale+shift is
    exactly zero on every fifth element (and wherever z happens to meet the channel's zero point), positive and negative
    elsewhere; y holds exact zeros beside positives and negatives."""
    z0 = (rng.integers(-8, 9, size=C) / 4.0).astype(np.float32)                       # zero point, multiples of 1/4
    scale = (rng.choice([-1.0, 1.0], size=C) * rng.choice([0.5, 1.0, 2.0, 4.0], size=C)).astype(np.float32)
    shift = (-z0 * scale).astype(np.float32)                                           # multiples of 1/8, |.| <= 8
    z = dyadic(rng, (rows, C))
    flat = z.reshape(-1)
    flat[::5] = np.broadcast_to(z0, (rows, C)).reshape(-1)[::5]
    y = dyadic(rng, (rows, C), lim=3)                                                  # {-3..3}/8: a seventh are zeros
    dy = dyadic(rng, (rows, C), lim=16)
    mean = dyadic(rng, C)
    invstd = rng.choice([0.5, 1.0, 2.0], size=C).astype(np.float32)
    k0 = (rng.choice([-1.0, 1.0], size=C) * rng.choice([0.5, 1.0, 2.0], size=C)).astype(np.float32)
    k1 = (rng.choice([-1.0, 1.0], size=C) * rng.choice([0.25, 0.5, 1.0], size=C)).astype(np.float32)
    k2 = dyadic(rng, C)
    return dict(z=z, y=y, dy=dy, scale=scale, shift=shift, mean=mean, invstd=invstd, k0=k0, k1=k1, k2=k2)


def normal_bn(rng, rows, C):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(z=f(rows, C) * 3 + f(C) * 2, y=f(rows, C), dy=f(rows, C), scale=f(C), shift=f(C), mean=f(C) * 2,
                invstd=(np.abs(f(C)) + 0.25).astype(np.float32), k0=f(C), k1=f(C), k2=f(C))


def bn_data(kind, rng, rows, C):
    return dyadic_bn(rng, rows, C) if kind == "dyadic" else normal_bn(rng, rows, C)


def affine_data(kind, rng, rows, C):
    """x, res and the two per-channel affines.  Dyadic: x*scale+shift has exact zeros (see dyadic_bn); the residual affine
    is again power-of-two scales and k/8 shifts."""
    d = bn_data(kind, rng, rows, C)
    e = bn_data(kind, rng, rows, C)
    return dict(x=d["z"], scale=d["scale"], shift=d["shift"], res=e["z"], rscale=e["scale"], rshift=e["shift"])


# --------------------------------------------------------------------------------------------------------------------
# float64 references.  Every one returns (reference, sum of the absolute values of the terms of each element)
# --------------------------------------------------------------------------------------------------------------------
def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def ref_affine_act(x, scale, shift, res, rscale, rshift, relu):
    x = f64(x)
    v, terms = x, np.abs(x)
    if scale is not None:
        v, terms = x * f64(scale) + f64(shift), np.abs(x * f64(scale)) + np.abs(f64(shift))
    if res is not None:
        t, tt = f64(res), np.abs(f64(res))
        if rscale is not None:
            t, tt = f64(res) * f64(rscale) + f64(rshift), np.abs(f64(res) * f64(rscale)) + np.abs(f64(rshift))
        v, terms = v + t, terms + tt
    if relu:
        v = np.maximum(v, 0.0)
    return v, terms


def ref_mask(mask_mode, z, y, scale, shift):
    """The strict > 0 mask: none, of the ReLU output y, or of the recomputed pre-activation z*scale+shift."""
    if mask_mode == 0:
        return np.ones(np.shape(z), dtype=bool)
    if mask_mode == 1:
        return f64(y) > 0
    return f64(z) * f64(scale) + f64(shift) > 0


def ref_bn_bwd_terms(d, mask_mode):
    """The two per-element contributions of dj_bn_bwd_reduce: masked dy, and masked dy * (z - mean) * invstd."""
    g = np.where(ref_mask(mask_mode, d["z"], d["y"], d["scale"], d["shift"]), f64(d["dy"]), 0.0)
    return g, g * (f64(d["z"]) - f64(d["mean"])) * f64(d["invstd"])


def ref_bn_bwd_apply(d, mask_mode):
    """dz = k0*g + k1*z + k2 and the masked gradient g; -> (dz, terms of dz, g)."""
    g = np.where(ref_mask(mask_mode, d["z"], d["y"], d["scale"], d["shift"]), f64(d["dy"]), 0.0)
    a, b, c = f64(d["k0"]) * g, f64(d["k1"]) * f64(d["z"]), np.broadcast_to(f64(d["k2"]), g.shape)
    return a + b + c, np.abs(a) + np.abs(b) + np.abs(c), g


def block_sums(v):
    """Per block of 64 rows: [ceil(rows/64)][C] sums of v and of |v|."""
    v = f64(v)
    rows, C = v.shape
    nblk = -(-rows // RB)
    pad = np.zeros((nblk * RB, C))
    pad[:rows] = v
    blk = pad.reshape(nblk, RB, C)
    return blk.sum(1), np.abs(blk).sum(1)


def ref_partials(v0, v1):
    """[nblk][2][C] partial rows of a column reduction with their term sums."""
    s0, a0 = block_sums(v0)
    s1, a1 = block_sums(v1)
    return np.stack([s0, s1], 1), np.stack([a0, a1], 1)


# one partial-row entry: 64 fp32 additions (63 of the rows and lanes, rounded up) plus the roundings of the term itself
# (at most 3: x*x has one, g*(z-mean)*invstd three, dy*x*rnorm two) -> 68 U times the sum of the absolute terms
PARTIAL_BOUND = 68 * U
# an elementwise result: at most four roundings (two affines of one product and one sum each fuse or round separately, one
# sum of the two, k0*g + k1*z + k2 likewise) -> 4 U times the sum of the absolute terms of that element
ELEMENTWISE_BOUND = 4 * U


def fin_partials(rng, nrows, C, special=True):
    """Synthetic fp32 partial rows [nrows][2][C] of a (sum, sum of squares) reduction over 64 pixels per row, so count =
    64*nrows.  Slot 1 is at least slot0^2/64 + 32, which keeps the variance positive.  With `special`, column 0 is what a
    constant input 3.0 leaves (variance exactly 0), and column 1 (if there is one) has q/n - m^2 < 0 (the clamp)."""
    s = (rng.standard_normal((nrows, C)) * 40).astype(np.float32)
    q = (s.astype(np.float64) ** 2 / RB + RB * rng.uniform(0.5, 1.5, (nrows, C))).astype(np.float32)
    if special:
        s[:, 0], q[:, 0] = 192.0, 576.0
        if C > 1:
            s[:, 1], q[:, 1] = 192.0, 575.5
    return np.stack([s, q], 1)


def ref_bn_train_finalize(partial, count, conv_bias, gamma, beta, eps, momentum, moving_mean, moving_var):
    """The finalizer's formula in float64 on the GIVEN fp32 partials.  -> dict name -> (reference, bound).
    Bounds: ULP*|ref| for a double stored as a float; one more ULP of each operand term per further fp32 operation."""
    p = f64(partial)
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    m = s / count
    var = np.maximum(q / count - m * m, 0.0)
    mean = m + (f64(conv_bias) if conv_bias is not None else 0.0)
    invstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    sc = f64(gamma) * invstd
    shift = f64(beta) - mean * sc
    out = {
        "save_mean": (mean, ULP * np.abs(mean)),                      # 1: the store
        "save_invstd": (invstd, ULP * np.abs(invstd)),                # 1: the store
        "scale": (sc, 2 * ULP * np.abs(sc)),                          # 2: invstd stored, gamma*invstd
        # 5: (float)mean, sc (2), their product -> 4 on |mean*sc|; the subtraction -> 1 on |shift|
        "shift": (shift, ULP * (4 * np.abs(mean * sc) + np.abs(shift))),
    }
    if moving_mean is not None:
        mom = float(np.float32(momentum))
        unbiased = var * (count / (count - 1.0 if count > 1 else 1.0))
        nm = f64(moving_mean) * mom + mean * (1.0 - mom)
        nv = f64(moving_var) * mom + unbiased * (1.0 - mom)
        # old*momentum: 1; (float)stat, 1.f - momentum, their product: 3; the sum: 1 on the result
        out["moving_mean"] = (nm, ULP * (np.abs(f64(moving_mean) * mom) + 3 * np.abs(mean * (1 - mom)) + np.abs(nm)))
        out["moving_var"] = (nv, ULP * (np.abs(f64(moving_var) * mom) + 3 * np.abs(unbiased * (1 - mom)) + np.abs(nv)))
    return out


def ref_bn_bwd_finalize(partial, count, gamma, mean, invstd):
    """All five outputs are doubles stored once: ULP*|ref| each (1 operation)."""
    p = f64(partial)
    sb, sg = p[:, 0].sum(0), p[:, 1].sum(0)
    is_, sc = f64(invstd), f64(gamma) * f64(invstd)
    c1, c2 = sb / count, sg / count
    vals = {"dbeta": sb, "dgamma": sg, "k0": sc, "k1": -sc * c2 * is_, "k2": -sc * c1 + sc * c2 * f64(mean) * is_}
    return {k: (v, ULP * np.abs(v)) for k, v in vals.items()}


def ref_colreduce_finalize(partial, which, out_before, beta):
    """out (+)= column sum of slot `which`: the double stored once (1), plus the fp32 addition with beta (1 more)."""
    s = f64(partial)[:, which].sum(0)
    if not beta:
        return s, ULP * np.abs(s)
    r = s + f64(out_before)
    return r, ULP * (np.abs(s) + np.abs(r))


def ref_bn_infer_coeffs(gamma, beta, moving_mean, moving_var, eps):
    """scale = gamma * rsqrtf(var + eps): 3 fp32 operations, the addition, rsqrtf (accurate to ONE ulp on this device: the
    allowance for it is ULP where a correctly rounded operation would get U) and the product -> 3 ULP |scale|.
    shift = beta - mean*scale: the product on top of scale's three -> 4 ULP |mean*scale|, the subtraction -> ULP |shift|."""
    sc = f64(gamma) / np.sqrt(f64(moving_var) + float(np.float32(eps)))
    sh = f64(beta) - f64(moving_mean) * sc
    return {"scale": (sc, 3 * ULP * np.abs(sc)), "shift": (sh, ULP * (4 * np.abs(f64(moving_mean) * sc) + np.abs(sh)))}


def ref_colsum(x, out_before, beta):
    """dj_colsum_direct / _multi: double accumulation, one store (1), one fp32 addition with beta (1 more)."""
    s = f64(x).sum(0)
    if not beta:
        return s, ULP * np.abs(s)
    r = s + f64(out_before)
    return r, ULP * (np.abs(s) + np.abs(r))


def ref_upsample2x(x):
    """y[b, 2i+a, 2j+c, :] = x[b, i, j, :] as a plain loop."""
    B, H, W, C = x.shape
    y = np.empty((B, 2 * H, 2 * W, C), dtype=x.dtype)
    for b in range(B):
        for oh in range(2 * H):
            for ow in range(2 * W):
                y[b, oh, ow] = x[b, oh // 2, ow // 2]
    return y


# --------------------------------------------------------------------------------------------------------------------
# multi-part launches
# --------------------------------------------------------------------------------------------------------------------
# (rows, cols, ld_src, ld_dst, src_off, dst_off): 4-wide-able parts mixed with scalar ones; the largest is scalar (the grid
# is sized for it); the smallest is one element
COPY_PARTS_TABLE = [
    (37, 23, 25, 29, 0, 1),      # scalar, 851 elements: the largest
    (1, 1, 1, 1, 0, 0),          # a single element
    (16, 8, 8, 16, 0, 4),        # 4-wide, destination a channel slice
    (5, 12, 12, 12, 0, 0),       # 4-wide dense
    (9, 8, 12, 12, 2, 0),        # scalar: source base misaligned
    (3, 4, 5, 8, 0, 0),          # scalar: ld_src % 4 != 0
    (64, 4, 4, 8, 4, 4),         # 4-wide
    (2, 7, 7, 9, 0, 0),          # scalar: cols % 4 != 0
    (11, 16, 20, 24, 4, 8),      # 4-wide (the ninth part: a second launch)
]
COPY_PART_COUNTS = [1, 8, 9]


def copy_part_v4(part):
    rows, cols, lds, ldd, so, do = part
    return cols % 4 == 0 and lds % 4 == 0 and ldd % 4 == 0 and aligned16(so) and aligned16(do)


# (rows, C, ld): parts of mixed C, so that the blocks past a small part's C take the early return
COLSUM_PARTS_TABLE = [(193, 40, 44), (1, 1, 1), (64, 16, 16), (257, 17, 19), (37, 5, 9), (300, 3, 8), (65, 33, 33)]
COLSUM_PART_COUNTS = [1, 32, 33]


def colsum_parts(n):
    return [COLSUM_PARTS_TABLE[i % len(COLSUM_PARTS_TABLE)] for i in range(n)]


# --------------------------------------------------------------------------------------------------------------------
# L2Normalization
# --------------------------------------------------------------------------------------------------------------------
L2_ZERO_ROW = 0
L2_CLAMP_ROWS = (1, 6)        # 0 < sum x^2 < 1e-13: the clamp holds, and the two branches of the backward differ
L2_ABOVE_ROWS = (2, 9)        # sum x^2 in [1e-10, 1e-8]: just above the clamp (1e-12)


def l2_input(C, seed=0):
    rng = np.random.default_rng(1000 + C + seed)
    x = (rng.standard_normal((L2_ROWS, C)) * 4).astype(np.float32)
    x[L2_ZERO_ROW] = 0.0
    unit = rng.standard_normal((L2_ROWS, C))
    unit /= np.sqrt((unit * unit).sum(1, keepdims=True))
    for r, ss in zip(L2_CLAMP_ROWS, (9e-14, 5e-14)):
        x[r] = (unit[r] * np.sqrt(ss)).astype(np.float32)
    for r, ss in zip(L2_ABOVE_ROWS, (1e-9, 4e-10)):
        x[r] = (unit[r] * np.sqrt(ss)).astype(np.float32)
    gamma = (rng.uniform(18, 23, C)).astype(np.float32)
    dy = rng.standard_normal((L2_ROWS, C)).astype(np.float32)
    for r in L2_CLAMP_ROWS:     # gradients along x: the projection that a clamped row must NOT subtract is large
        dy[r] = np.abs(dy[r]) * np.sign(x[r])
    dx0 = rng.standard_normal((L2_ROWS, C)).astype(np.float32)
    return x, gamma, dy, dx0


def l2_sumsq(x, dtype):
    """Row sums of squares accumulated in `dtype`, one element after the other."""
    x = np.asarray(x, dtype=dtype)
    ss = np.zeros(x.shape[0], dtype=dtype)
    for c in range(x.shape[1]):
        ss = (ss + x[:, c] * x[:, c]).astype(dtype)
    return ss


def l2_rel(C, rsqrt_uses=1):
    """Relative allowance of an L2Normalization result against the largest term of its row.  A row reduction over C
    elements in fp32 (sum of squares, or the dot product of the backward) makes at most C additions and three roundings per
    term in whatever order: (C + 3) U relative to the sum of the absolute terms, C + 4 with the final product; 8 U (C + 4)
    also covers the error of rnorm = rsqrt(ss) entering a term up to three times (x*rn, the dot, rn * ...) at half the
    relative error of ss each.  rsqrtf itself is accurate to one ulp: ULP for each time rnorm enters a term -- once in y,
    in rnorm and in a dgamma term, three times in rn * xhat * sum(g * xhat) of dx."""
    return 8 * U * (C + 4) + rsqrt_uses * ULP


# --------------------------------------------------------------------------------------------------------------------
# max pooling
# --------------------------------------------------------------------------------------------------------------------
PoolCase = collections.namedtuple("PoolCase", "name H W kh kw sh sw pt pl OH OW")
POOL_B = 2
POOL_GEOMS = [
    PoolCase("3x3s1p1", 5, 7, 3, 3, 1, 1, 1, 1, 5, 7),
    PoolCase("3x3s2p0", 5, 7, 3, 3, 2, 2, 0, 0, 3, 4),            # trailing taps past the edge only
    PoolCase("3x3s2same6x7", 6, 7, 3, 3, 2, 2, 0, 1, 3, 4),       # TF 'same' of an even and an odd extent: pt 0, pl 1
    PoolCase("2x2s2valid", 5, 7, 2, 2, 2, 2, 0, 0, 2, 3),
    PoolCase("2x2s3gaps", 5, 7, 2, 2, 3, 3, 0, 0, 2, 2),          # rows 2 and columns 2, 5, 6 belong to no window
    # windows and strides that differ between the axes: an H/W swap of either changes the output shape
    PoolCase("2x3s1x2", 5, 7, 2, 3, 1, 2, 0, 0, 4, 3),
    PoolCase("3x2s2x1same", 6, 7, 3, 2, 2, 1, 0, 0, 3, 7),        # TF 'same': one trailing pad row and column, none in front
]
POOL_ANISOTROPIC = ("2x3s1x2", "3x2s2x1same")
POOL_C = [4, 6]
POOL_DATA = ["mixed", "negative", "relu"]
POOL_ARGMAX = [None, 0, 1]      # no saved arg-max, saved at byte offset 0, saved at byte offset 1


def pool_input(geom, C, data):
    rng = np.random.default_rng(77 + geom.H * 100 + C * 10 + POOL_DATA.index(data))
    x = (rng.integers(-6, 7, size=(POOL_B, geom.H, geom.W, C)) / 8.0).astype(np.float32)    # few values: many ties
    if data == "negative":
        x = (-np.abs(x) - 0.125).astype(np.float32)
    elif data == "relu":
        x = np.maximum(x - 0.5, 0).astype(np.float32)      # mostly zeros: whole windows tie, with and without pad taps
    dy = (rng.integers(-16, 17, size=(POOL_B, geom.OH, geom.OW, C)) / 8.0).astype(np.float32)
    dx0 = (rng.integers(-16, 17, size=x.shape) / 8.0).astype(np.float32)
    return x, dy, dx0


def ref_maxpool(x, geom, pad_zero):
    """First maximum in row-major window order, as a plain window loop.  -> (y, code): code is the window-relative tap of
    the winner, 255 where a zero pad tap won."""
    B, H, W, C = x.shape
    y = np.empty((B, geom.OH, geom.OW, C), dtype=np.float64)
    code = np.empty((B, geom.OH, geom.OW, C), dtype=np.uint8)
    for b in range(B):
        for oh in range(geom.OH):
            for ow in range(geom.OW):
                for c in range(C):
                    best, tap = -np.inf, 255
                    for i in range(geom.kh):
                        for j in range(geom.kw):
                            hh, ww = oh * geom.sh + i - geom.pt, ow * geom.sw + j - geom.pl
                            inside = 0 <= hh < H and 0 <= ww < W
                            if not inside and not pad_zero:
                                continue
                            v = float(x[b, hh, ww, c]) if inside else 0.0
                            if v > best:
                                best, tap = v, (i * geom.kw + j if inside else 255)
                    y[b, oh, ow, c], code[b, oh, ow, c] = best, tap
    return y, code


def ref_maxpool_bwd(code, dy, geom, x_shape):
    """Scatter of dy to the winning taps (nothing for code 255), in float64."""
    dx = np.zeros(x_shape, dtype=np.float64)
    B, OH, OW, C = code.shape
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                for c in range(C):
                    t = int(code[b, oh, ow, c])
                    if t == 255:
                        continue
                    hh, ww = oh * geom.sh + t // geom.kw - geom.pt, ow * geom.sw + t % geom.kw - geom.pl
                    dx[b, hh, ww, c] += float(dy[b, oh, ow, c])
    return dx


def pool_uncovered(geom):
    """Input pixels (h, w) that belong to no window."""
    cov = np.zeros((geom.H, geom.W), dtype=bool)
    for oh in range(geom.OH):
        for ow in range(geom.OW):
            for i in range(geom.kh):
                for j in range(geom.kw):
                    hh, ww = oh * geom.sh + i - geom.pt, ow * geom.sw + j - geom.pl
                    if 0 <= hh < geom.H and 0 <= ww < geom.W:
                        cov[hh, ww] = True
    return ~cov


# --------------------------------------------------------------------------------------------------------------------
# the table of paths the GPU tests must reach: name -> a predicate-checked witness, filled by `path_witnesses`
# --------------------------------------------------------------------------------------------------------------------
def path_witnesses():
    """-> dict path name -> list of case descriptions that reach it, each checked against the predicates above."""
    w = collections.defaultdict(list)
    for l in LAYOUTS:
        slabs = layout_slabs(l, 3)
        w["ew_" + ("v4" if v4(l.C, slabs, (l.vec_off,)) else "scalar") + ":" + l.name].append(l)
    for C in COLRED_C_V4:
        w["colreduce_v4_tx%d_cb%d" % (tx_log2(C, True), column_blocks(C, True))].append(C)
    for C in COLRED_C_SCALAR:
        w["colreduce_scalar_tx%d_cb%d" % (tx_log2(C, False), column_blocks(C, False))].append(C)
    for n in FIN_NROWS:
        w[fin_path(n)].append(n)
    for C in POOL_C:
        for am in POOL_ARGMAX:
            w["pool_" + ("fwd4" if pool4(C, 4, 4, am) else "fwd_scalar")].append((C, am))
            w["pool_" + pool_bwd_path(C, 4, 4, am)].append((C, am))
    for n in COPY_PART_COUNTS:
        parts = COPY_PARTS_TABLE[:n]
        w["copy_multi_%s" % ("mixed" if len({copy_part_v4(p) for p in parts}) == 2 else
                             "v4" if copy_part_v4(parts[0]) else "scalar")].append(n)
    return dict(w)


REQUIRED_PATHS = (
    ["ew_v4:v4_dense", "ew_v4:v4_slice"] + ["ew_scalar:" + n for n in PATH_REASONS if n.startswith("scalar")]
    + ["colreduce_v4_tx%d_cb1" % t for t in (2, 3, 4, 5)] + ["colreduce_v4_tx6_cb2"]
    + ["colreduce_scalar_tx2_cb1", "colreduce_scalar_tx3_cb1", "colreduce_scalar_tx5_cb1", "colreduce_scalar_tx6_cb2"]
    # fin_trips<lane 0>_<lane 63>_tail<lane 0>_<lane 63>: no unrolled loop (1 and 192 rows), lane 0 alone in it (193),
    # every lane in it and no tail (256), a one-row tail (257), two iterations beside one (449), two and a tail (704)
    + ["fin_trips0_0_tail1_0", "fin_trips0_0_tail3_3", "fin_trips1_0_tail0_3", "fin_trips1_1_tail0_0",
       "fin_trips1_1_tail1_0", "fin_trips2_1_tail0_3", "fin_trips2_2_tail3_3"]
    + ["pool_fwd4", "pool_fwd_scalar", "pool_bwd4", "pool_bwd_saved_scalar", "pool_bwd_rescan"]
    + ["copy_multi_scalar", "copy_multi_mixed"]
)
