"""Cases shared by tests/test_conv_geometry_cases_cpu.py, tests/test_conv_anisotropic_gpu.py and
tests/test_conv_generic_gpu.py: convolution geometries that differ between the two axes, the smallest geometries that
reach each path of the generic implicit-GEMM kernel (dj_igemm_kernel, csrc/dj_igemm.h), their fp64 oracle, and a Python
restatement of what the launchers decide for them (csrc/dj_conv.hip, fast_mode and dj_gather_variant of
csrc/dj_conv_launch.h) -- a second statement of that contract, as pool4() of tests/norm_edge_cases.py is for the pooling
launchers.  No GPU is imported here.

A geometry is (batch, H, W, Cin, Cout, kernel, strides, padding, dilation); kernel, strides and dilation are (h, w) pairs
or one int for both; padding is "valid", "same" or ((top, bottom), (left, right))."""
import collections
import functools

import torch

from oracle import keras_ops as ko

DJ_BK = 32                                        # K-step of the fp32 kernels
TILES = [(128, 128), (128, 64), (64, 64), (128, 32)]     # tile indices 0-3 (kCfgs of dj_conv_launch.h)
N_CFG = 14
# what the indices [0, N_CFG) name on the generic kernel, which ignores the schedule variants (dj_launch_cfg)
GENERIC_TILE_OF_CFG = [0, 1, 2, 3, 0, 1, 2, 2, 1, 0, 1, 2, 2, 1]
ROLES = ("fwd", "dgrad", "wgrad")


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def norm(geom):
    """-> the geometry with kernel, strides and dilation as pairs."""
    b, h, w, ci, co, k, s, pad, d = geom
    return (b, h, w, ci, co, pair(k), pair(s), pad, pair(d))


def explicit_pads(geom):
    """-> ((top, bottom), (left, right)) as Keras resolves the geometry's padding."""
    b, h, w, ci, co, k, s, pad, d = norm(geom)
    if pad == "valid":
        return ((0, 0), (0, 0))
    if pad == "same":
        pt, pb, _ = ko.same_padding(h, k[0], s[0], d[0])
        pl, pr, _ = ko.same_padding(w, k[1], s[1], d[1])
        return ((pt, pb), (pl, pr))
    return (tuple(pad[0]), tuple(pad[1]))


def out_size(geom):
    b, h, w, ci, co, k, s, pad, d = norm(geom)
    (pt, pb), (pl, pr) = explicit_pads(geom)
    return (ko.valid_out_size(h + pt + pb, k[0], s[0], d[0]), ko.valid_out_size(w + pl + pr, k[1], s[1], d[1]))


# --------------------------------------------------------------------------------------------------------------------
# where the tensors of a case lie: pixel strides (None: dense) and byte offsets of x, of y / dy and of the weights
# --------------------------------------------------------------------------------------------------------------------
Layout = collections.namedtuple("Layout", "name ld_x off_x ld_y off_y off_w")
DENSE = Layout("dense", None, 0, None, 0, 0)
VIEW67 = Layout("view67", 67, 4, 67, 4, 0)        # x, y and dy are views [..., 1:65] of 67-channel buffers
W_OFF4 = Layout("w_off4", None, 0, None, 0, 4)    # the weights start 4 bytes past a 16-byte boundary

# One case: the geometry, its layout, what it is there for, and what the launchers make of it --
#   route[role] = "fast" (the branch-free kernels) or "generic:<A><B>" with v / s for the vector / scalar operand path;
#   the input gradient of a strided 1x1 convolution with equal strides is "scatter:..." (cmap = 1)
#   np = gather variants (fwd, dgrad, wgrad on a 128-row tile, wgrad on a 64-row tile) of the roles that are "fast"
Case = collections.namedtuple("Case", "geom layout why route np")


def _c(geom, why, fwd, dgrad, wgrad, np=(None, None, None, None), layout=DENSE):
    return Case(geom, layout, why, {"fwd": fwd, "dgrad": dgrad, "wgrad": wgrad}, np)


def case_id(case):
    """A test id that tells the cases apart: extents, kernel, strides, dilation, layout."""
    b, h, w, ci, co, k, s, pad, d = norm(case.geom)
    return "%dx%dx%dx%dx%d-k%dx%d-s%dx%d-d%dx%d-%s" % ((b, h, w, ci, co) + k + s + d + (case.layout.name,))


ANISOTROPIC = [
    _c((2, 7, 10, 64, 96, (1, 3), (1, 1), "same", (1, 1)), "pad_top 0, pad_left 1",
       "fast", "fast", "fast", (2, 2, 0, 3)),
    _c((2, 10, 7, 64, 96, (3, 1), (1, 1), "same", (1, 1)), "pad_top 1, pad_left 0",
       "fast", "fast", "fast", (2, 2, 0, 3)),
    _c((2, 9, 12, 128, 64, (2, 3), (1, 1), "same", (1, 1)), "even x odd kernel; Cin % 128 == 0: pixel-walk wgrad",
       "fast", "fast", "fast", (2, 2, 3, 3)),
    # (9 columns, not 8: an output row must not divide the 16 / 32 pixels of a K-step, or the walk never takes its row carry)
    _c((2, 11, 9, 64, 64, (3, 3), (2, 1), "same", (1, 1)),
       "stride (2,1): strided input gradient on the generic division path; walk carries with sH != sW",
       "fast", "generic:vv", "fast", (2, None, 0, 3)),
    _c((2, 8, 11, 64, 64, (3, 3), (1, 2), "same", (1, 1)), "stride (1,2)",
       "fast", "generic:vv", "fast", (2, None, 0, 3)),
    _c((1, 12, 9, 128, 64, (3, 3), (1, 1), "same", (1, 3)), "dilation (1,3): pads 1 / 3",
       "fast", "fast", "fast", (2, 2, 3, 3)),
    _c((1, 9, 12, 128, 64, (3, 2), (1, 1), "same", (2, 1)), "dilation (2,1): pads 2 / 0",
       "fast", "fast", "fast", (2, 2, 3, 3)),
    _c((2, 8, 9, 64, 64, (1, 1), (2, 1), "valid", (1, 1)),
       "1x1 with unequal strides: NOT the scatter form; the bounds-free variant (NP 1) is refused for the weight gradient",
       "fast", "generic:vv", "fast", (1, None, 0, 3)),
    _c((2, 8, 9, 64, 64, (1, 1), (1, 2), "valid", (1, 1)), "1x1, strides (1,2)",
       "fast", "generic:vv", "fast", (1, None, 0, 3)),
    _c((2, 7, 9, 64, 32, (3, 2), (1, 1), ((2, 0), (0, 1)), (1, 1)), "explicit one-sided pads",
       "fast", "fast", "fast", (2, 2, 0, 3)),
    _c((2, 6, 9, 24, 20, (3, 2), (2, 1), "same", (1, 1)), "generic kernel, vector paths (the weight gradient needs Cin % 4 only)",
       "generic:vv", "generic:vv", "fast", (None, None, 0, 0)),
    _c((2, 5, 8, 6, 21, (2, 3), (1, 2), "same", (2, 1)), "generic kernel, every scalar path",
       "generic:ss", "generic:ss", "generic:ss"),
]

# Conv2DTranspose(filters, kernel, strides) on a (batch, H, W, Cin) input, run as the input gradient of the convolution it
# transposes: (batch, H, W, Cin, filters, kernel, strides)
TRANSPOSE = [
    (2, 5, 4, 32, 24, (2, 3), (2, 3)),      # windows tile the output: every output pixel has one tap
    (2, 5, 6, 32, 24, (3, 3), (2, 1)),      # overlapping windows, one to three taps per output pixel
]


def transpose_conv_geom(tcase):
    """The convolution whose input gradient is the transposed layer: its input is the layer's output."""
    b, h, w, ci, co, k, s = tcase
    oh, ow = (h - 1) * s[0] + k[0], (w - 1) * s[1] + k[1]
    return (b, oh, ow, co, ci, k, s, "valid", (1, 1))


GENERIC = [
    _c((2, 9, 11, 3, 20, 3, 1, "same", 1),
       "fwd scalar A; wgrad scalar A with M' = 27 (smaller than any tile); dgrad vector with srcC % 32 != 0",
       "generic:sv", "generic:vv", "generic:sv"),
    _c((2, 7, 5, 64, 126, 3, 1, "same", 1),
       "fwd vector A / scalar B with an N tail; dgrad scalar A (dj_gather_elem) and scalar B (B-mode 1); wgrad scalar B",
       "generic:vs", "generic:ss", "generic:vs"),
    _c((3, 6, 7, 24, 20, 3, 1, "same", 1), "all-vector generic, 126 rows",
       "generic:vv", "generic:vv", "fast", (None, None, 0, 0)),
    _c((2, 17, 19, 24, 128, 3, 1, "same", 1),
       "fwd: full 128x128 tiles and a partial one, K = 216 (the K tail in the 7th K-step); generic by Cin % 32",
       "generic:vv", "fast", "fast", (None, 2, 0, 0)),
    _c((2, 17, 19, 128, 24, 3, 1, "same", 1),
       "dgrad: the same, generic by Cout % 32; the BatchNormalization-backward-statistics epilogue",
       "fast", "generic:vv", "fast", (2, None, 3, 3)),
    _c((2, 11, 13, 64, 64, 3, 2, "same", 1), "strided 3x3 input gradient (generic by stride)",
       "fast", "generic:vv", "fast", (2, None, 0, 3)),
    _c((2, 12, 12, 4, 32, 7, 2, ((3, 3), (3, 3)), 1), "one K-step spans eight taps",
       "generic:vv", "generic:vv", "fast", (None, None, 0, 0)),
    _c((2, 8, 8, 64, 24, 1, 2, "valid", 1), "strided-1x1 scatter (cmap 1) on the generic kernel, vector",
       "fast", "scatter:generic:vv", "fast", (1, None, 0, 3)),
    _c((2, 8, 8, 64, 21, 1, 2, "valid", 1), "strided-1x1 scatter on the generic kernel, scalar",
       "generic:vs", "scatter:generic:ss", "generic:vs"),
    _c((2, 10, 10, 64, 64, 3, 1, "same", 1),
       "eligible dimensions, but x / y / dy are views [..., 1:65] of 67-channel buffers: generic by alignment only",
       "generic:sv", "generic:sv", "generic:ss", layout=VIEW67),
    _c((2, 10, 10, 64, 64, 3, 1, "same", 1),
       "eligible dimensions and dense tensors, the weights 4 bytes past a 16-byte boundary: vector A beside scalar B "
       "in the input gradient, which no channel count gives (both follow Cout % 4)",
       "generic:vs", "generic:vs", "fast", (None, None, 0, 3), layout=W_OFF4),
]


# what tests/test_conv_generic_gpu.py runs: the square cases and the two anisotropic ones that live on the generic kernel
# (the only forward GEMM with both operands on the scalar path is among the latter)
GENERIC_KERNEL_CASES = GENERIC + [c for c in ANISOTROPIC if c.why.startswith("generic kernel")]


# --------------------------------------------------------------------------------------------------------------------
# the launchers' decisions, restated
# --------------------------------------------------------------------------------------------------------------------
def aligned16(byte_off):
    return byte_off % 16 == 0


def dgrad_is_strided_1x1(geom):
    b, h, w, ci, co, k, s, pad, d = norm(geom)
    (pt, _), (pl, _) = explicit_pads(geom)
    return k == (1, 1) and pt == 0 and pl == 0 and (s[0] > 1 or s[1] > 1) and s[0] == s[1]


Launch = collections.namedtuple("Launch", "am bmd M N K srcC vecA vecB fast scatter gather")


def launch(role, geom, layout=DENSE, prologue=False, allow_fast=True, bias=False):
    """What dj_conv2d_nhwc_fwd / _dgrad / _wgrad set up for fp32 tensors: the GEMM role (A-mode, B-mode), its extents,
    vecA / vecB, the result of fast_mode<AM, BMD> (0 generic, 1 branch-free, 2 branch-free with the affine prologue) and
    whether the input gradient takes the strided-1x1 scatter form.  `gather`: the fields dj_gather_variant looks at."""
    b, h, w, ci, co, k, s, pad, d = norm(geom)
    (pt, _), (pl, _) = explicit_pads(geom)
    oh, ow = out_size(geom)
    ld_x, ld_y = layout.ld_x or ci, layout.ld_y or co
    ax, ay, aw = aligned16(layout.off_x), aligned16(layout.off_y), aligned16(layout.off_w)
    taps = k[0] * k[1]
    scatter = False
    gather = dict(KH=k[0], KW=k[1], pT=pt, pL=pl, sH=s[0], sW=s[1], rowH=oh, rowW=ow, srcH=h, srcW=w)
    if role == "fwd":
        am, bmd, M, N, K, srcC, ldb = 0, 0, b * oh * ow, co, taps * ci, ci, co
        vecA = ci % 4 == 0 and ld_x % 4 == 0 and ax
        vecB = co % 4 == 0 and aw
    elif role == "wgrad":
        am, bmd, M, N, K, srcC, ldb = 2, 0, taps * ci, co, b * oh * ow, ci, ld_y
        vecA = ci % 4 == 0 and ld_x % 4 == 0 and ax
        vecB = co % 4 == 0 and ld_y % 4 == 0 and ay
    else:
        assert role == "dgrad"
        vecA = co % 4 == 0 and ld_y % 4 == 0 and ay
        vecB = co % 4 == 0 and aw
        srcC, ldb = co, co
        scatter = dgrad_is_strided_1x1(geom) and not bias
        if scatter:      # a compact GEMM over the output grid, its rows scattered to the strided input pixels
            am, bmd, M, N, K = 0, 1, b * oh * ow, ci, co
            gather = dict(KH=1, KW=1, pT=0, pL=0, sH=1, sW=1, rowH=oh, rowW=ow, srcH=oh, srcW=ow)
        else:
            am, bmd, M, N, K = 1, 1, b * h * w, ci, taps * co
            gather.update(rowH=h, rowW=w, srcH=oh, srcW=ow)
    gather["srcC"] = srcC
    fast = 1
    if not allow_fast or not vecA or not vecB:
        fast = 0
    elif am != 2 and srcC % 32 != 0:
        fast = 0
    elif am != 2 and M >= (1 << 22):
        fast = 0
    elif am == 1 and s != (1, 1):
        fast = 0
    elif am == 2 and (srcC % 4 != 0 or K >= (1 << 24)):
        fast = 0
    elif bmd == 0 and (N % 4 != 0 or ldb % 4 != 0):
        fast = 0
    elif bmd == 1 and srcC % 32 != 0:
        fast = 0
    if fast and prologue:
        fast = 2
    return Launch(am, bmd, M, N, K, srcC, bool(vecA), bool(vecB), fast, scatter, gather)


def gather_variant(am, bm, g, variants=True, residual=False):
    """dj_gather_variant: 1 bounds-free 1x1, 2 tap cache (forward / input gradient), 3 pixel walk (weight gradient whose
    tiles lie under one tap each), 0 the plain kernel.  `variants`: dj_set_gather_variants."""
    if residual:
        return 0
    same_grid = am != 2 or (g["sH"] == 1 and g["sW"] == 1 and g["rowH"] == g["srcH"] and g["rowW"] == g["srcW"])
    if g["KH"] == 1 and g["KW"] == 1 and g["pT"] == 0 and g["pL"] == 0 and same_grid:
        return 1
    if not variants:
        return 0
    if am == 2:
        return 3 if g["srcC"] % bm == 0 else 0
    return 2


def route(role, geom, layout=DENSE, **kw):
    """The route string of a Case (see there) for one role."""
    l = launch(role, geom, layout, **kw)
    family = "fast" if l.fast else "generic:%s%s" % ("v" if l.vecA else "s", "v" if l.vecB else "s")
    return ("scatter:" if l.scatter else "") + family


def gather_variants_of(case):
    """(fwd, dgrad, wgrad on a 128-row tile, wgrad on a 64-row tile); None where the role is not branch-free."""
    out = []
    for role, bm in (("fwd", 128), ("dgrad", 128), ("wgrad", 128), ("wgrad", 64)):
        l = launch(role, case.geom, case.layout)
        out.append(gather_variant(l.am, bm, l.gather) if l.fast else None)
    return tuple(out)


def generic_coverage(cases=None):
    """What the generic cases reach when every role of every case runs on the generic kernel (the GPU test turns the
    branch-free kernels off for the roles that are eligible): a set of labels."""
    cov = set()
    for case in (GENERIC_KERNEL_CASES if cases is None else cases):
        for role in ROLES:
            l = launch(role, case.geom, case.layout, allow_fast=False)
            name = "scatter" if l.scatter else role
            cov.add("%s:A%s" % (name, "v" if l.vecA else "s"))
            cov.add("%s:B%s" % (name, "v" if l.vecB else "s"))
            cov.add("%s:A%sB%s" % (name, "v" if l.vecA else "s", "v" if l.vecB else "s"))
            if l.K % DJ_BK:
                cov.add("%s:ktail" % name)
            if l.am != 2 and l.srcC < DJ_BK and l.K > l.srcC:
                cov.add("%s:multitap" % name)
            if l.scatter:
                cov.add("cmap1")
            for bm, bn in TILES:
                if l.M >= bm and l.N >= bn:
                    cov.add("tile%dx%d:full" % (bm, bn))
                if l.M % bm or l.N % bn:
                    cov.add("tile%dx%d:edge" % (bm, bn))
                if l.M >= bm and l.N >= bn and (l.M % bm or l.N % bn):
                    cov.add("tile%dx%d:full+edge in one launch" % (bm, bn))
    return cov


REQUIRED_COVERAGE = (
    ["%s:A%sB%s" % (r, a, b) for r in ROLES for a in "vs" for b in "vs"]      # every A path x B path of every role
    + ["scatter:AvBv", "scatter:AsBs", "cmap1"]
    + ["fwd:ktail", "dgrad:ktail", "wgrad:ktail", "fwd:multitap", "dgrad:multitap"]
    + ["tile%dx%d:%s" % (bm, bn, what) for bm, bn in TILES for what in ("full", "edge", "full+edge in one launch")]
)


# --------------------------------------------------------------------------------------------------------------------
# operands and the fp64 oracle
# --------------------------------------------------------------------------------------------------------------------
def oracle_conv(x, wt, bias, geom):
    b, h, w, ci, co, k, s, pad, d = norm(geom)
    if isinstance(pad, tuple):
        x = ko.zero_padding(x, pad)
        pad = "valid"
    return ko.conv2d(x, wt, bias, s, pad, d)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def reference(geom):
    """Host operands and the fp64 oracle's results of one geometry: computed once, never written to.
    x, w, dy, bias, and a prologue (sc, sh) whose shift is larger in magnitude than the data and of both signs -- a padding
    pixel that is not zeroed AFTER the prologue shows.  y / dw: plain; y_pro / dw_pro: of relu(x * sc + sh); dx: of dy."""
    b, h, w, ci, co, k, s, pad, d = norm(geom)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, h, w, ci, generator=g)
    wt = torch.randn(k[0], k[1], ci, co, generator=g) * (2.0 / (k[0] * k[1] * ci)) ** 0.5
    sc = torch.rand(ci, generator=g) + 0.5
    # |shift| in [8, 9): above |x * scale| (< 1.5 * 5.5), both signs
    sh = (8.0 + torch.rand(ci, generator=g)) * torch.where(torch.rand(ci, generator=g) < 0.75, 1.0, -1.0)
    bias = torch.randn(co, generator=g)
    xa = torch.relu(x * sc + sh)
    xr, wr = xa.double().requires_grad_(True), wt.double().requires_grad_(True)
    yr = oracle_conv(xr, wr, None, geom)
    dy = torch.randn(*yr.shape, generator=g) * 1e-3
    yr.backward(dy.double())
    w_plain, x_plain = wt.double().requires_grad_(True), x.double().requires_grad_(True)
    y_plain = oracle_conv(x_plain, w_plain, None, geom)
    y_plain.backward(dy.double())
    host = {"x": x, "w": wt, "dy": dy, "sc": sc, "sh": sh, "bias": bias}
    ref = {"y_pro": yr.detach(), "y": y_plain.detach(), "dx": x_plain.grad, "dw_pro": wr.grad, "dw": w_plain.grad}
    return host, ref


def swapped_variants(geom):
    """The geometry with ONE of its pairs swapped between the axes -> [(what, geometry, weights transposed?)]; a pair
    whose halves are equal has no variant.  Swapping the kernel transposes the weight's first two axes with it, so that
    the taps keep their coefficients and only their positions move."""
    b, h, w, ci, co, k, s, pad, d = norm(geom)
    pads = explicit_pads(geom)
    out = []
    if s[0] != s[1]:
        out.append(("strides", (b, h, w, ci, co, k, s[::-1], pad, d), False))
    if d[0] != d[1]:
        out.append(("dilation", (b, h, w, ci, co, k, s, pad, d[::-1]), False))
    if pads[0] != pads[1]:
        out.append(("pads", (b, h, w, ci, co, k, s, (pads[1], pads[0]), d), False))
    if k[0] != k[1]:
        out.append(("kernel", (b, h, w, ci, co, k[::-1], s, pad, d), True))
    return out
