"""The exact operand-rounding model of the 16-bit-tile convolution GEMMs (csrc/dj_igemm_h16.h, PREC 1 / 2), the cases it
is checked on, and what each of them may be launched with.  Importable without a GPU: tests/test_lowp_model_cpu.py checks
the premises, tests/test_lowp_model_gpu.py holds the kernels to the model.

The model (dj_igemm_h16.h: header comment, dj_to_half4 / dj_to_bf16x4, dj_round4, store_a / store_b): the prologue runs in
fp32, every operand element is rounded ONCE (round-to-nearest-even) to the type T of the matrix instruction when it goes
to LDS, fp16 x fp16 and bf16 x bf16 products are exact in fp32, accumulation is fp32.  So a result is the fp64 convolution
of the ROUNDED operands up to fp32 accumulation: per element |got - model| <= (K + 2) u sum|a||b| with u = 2^-24, the bound
of a K-term fp32 sum of exact products in any order, plus u |result| per fp32 addition behind it (bias, `beta`, the
partial sums of a split reduction).  T per mode and GEMM (dj_launch_lowp_io): float16 = fp16 forward, bf16 gradients;
bfloat16 = bf16 everywhere.  A geometry outside the branch-free kernels' preconditions (fast_mode, dj_conv_launch.h) runs
the generic fp32 kernel in every mode: its model is the unrounded oracle, and 16-bit tensors are an error there.

Data.  A tensor that meets the kernel without a prologue is seeded randn (weights; gradients x 1e-3).  A tensor that goes
through a prologue lies on a grid on which the fp32 prologue is EXACT, whether or not the compiler contracts x*scale+shift
into an fma: x = k/1024 with |k| <= 4096, scale in {0.5, 1, 2}, shift = j/1024 with |j| <= 512 (products are multiples of
1/2048 below 8, sums of two affine terms below 18: 16 significant bits).  Random data does not do: 1.1e-4 of fp16 operands
round differently after fma and after mul + add, 3e-6 rel-L2.  The same grid carries the BatchNormalization input z of the
backward-statistics epilogue with its mean (j/1024) and inverse deviation ({0.5, 1, 2}): mask and x-hat are exact."""
import collections
import functools

import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U = 2.0 ** -24
REL_L2_BOUND = 2e-6          # the bound of the exact-fp32 MFMA kernels (tests/test_x3_gpu.py, tests/test_lowp_gpu.py)
MODES = ("float16", "bfloat16")

Geom = collections.namedtuple("Geom", "name b h w ci co k s pad dil")

# No geometry is larger than 2 x 12 x 12 x 256.  The first eight are the GEOMS of tests/test_gather_variants_gpu.py.
GEOMS = [
    # smallest non-square map whose row (5 pixels) is shorter than a K-step; 70 rows: M no multiple of 64; Cout 96: N tail
    Geom("map7x5", 2, 7, 5, 128, 96, 3, 1, "same", 1),
    # smallest map below one K-step of pixels: every K-step of the weight gradient carries into the next image
    Geom("map3x3", 3, 3, 3, 128, 64, 3, 1, "same", 1),
    # one-pixel map: eight of nine taps lie in the padding; M = 2, far below a tile
    Geom("map1x1", 2, 1, 1, 256, 64, 3, 1, "same", 1),
    # smallest stride-2 3x3 with an N tail (160 = 128 + 32): the input gradient is off the branch-free kernel (stride)
    Geom("stride2_ntail", 2, 9, 9, 128, 160, 3, 2, "same", 1),
    # dilation 6 on the smallest map where a tap still hits the image: most taps outside; 144 rows = two 128-row tiles
    Geom("dilation6", 1, 12, 12, 128, 64, 3, 1, "same", 6),
    # valid padding: the output grid is smaller than the input grid
    Geom("valid", 2, 6, 6, 128, 64, 3, 1, "valid", 1),
    # strided 1x1: the input gradient is the compact GEMM + scatter, the weight gradient gathers every second pixel
    Geom("strided1x1", 2, 8, 8, 256, 64, 1, 2, "valid", 1),
    # Cin = 192 = 3 x 64: 64-deep K-steps with a tap change every third step; Cin % 128 != 0
    Geom("cin192", 2, 6, 6, 192, 64, 3, 1, "same", 1),
    # even kernel: TensorFlow's `same` pads after only (pad_top = pad_left = 0, one row / column behind)
    Geom("k2_same", 2, 6, 5, 64, 96, 2, 1, "same", 1),
    # Cin % 64 != 0 and Cout % 64 != 0: launch_h16_depth falls back to 32-deep K-steps at run time, in both directions
    Geom("c96", 2, 5, 5, 96, 96, 3, 1, "same", 1),
    # smallest 1x1 stride-1 case (the residual-add form, the bounds-free NP 1 variant) with M = 162: two 128-row tiles,
    # M % 64 = 34, and Cin % 64 == 0
    Geom("pointwise", 2, 9, 9, 128, 96, 1, 1, "valid", 1),
    # OFF the branch-free preconditions (Cin % 32, Cout % 4): the generic fp32 kernel runs in every mode
    Geom("fallback", 2, 6, 6, 3, 126, 3, 1, "same", 1),
    # a strided 1x1 whose input gradient is off the preconditions (Cout % 32) while forward and weight gradient are on
    Geom("strided1x1_c48", 2, 4, 4, 32, 48, 1, 2, "valid", 1),
]
GEOM = {g.name: g for g in GEOMS}

FORMS = {
    "fwd": ("plain_bias_relu", "bn_stats", "slabs", "atomics", "addrelu_sum"),
    "dgrad": ("plain", "beta", "scatter", "bnb_masked", "bnb_unmasked", "transpose_bias"),
    "wgrad": ("plain", "pro"),
}

# Storage combinations: per direction, (name, types).  "w16" / "wbf" are the shadows of dj_shadow_weights; "@8": the shadow
# sits 8-byte (not 16-byte) aligned.  forward: (x, w, y); input gradient: (dy, w, dx); weight gradient: (x, dy).
STORAGE = {
    "fwd": (("f32", (F32, F32, F32)), ("x16_y16", (F16, F32, F16)), ("x32_y16", (F32, F32, F16)), ("x16_y32", (F16, F32, F32)),
            ("x16_w16@8_y16", (F16, F16, F16)), ("x32_w16_y32", (F32, F16, F32))),
    "dgrad": (("f32", (F32, F32, F32)), ("dybf_dxbf", (BF16, F32, BF16)), ("dy32_dxbf", (F32, F32, BF16)),
              ("dybf_dx32", (BF16, F32, F32)), ("dybf_wbf@8_dxbf", (BF16, BF16, BF16)), ("dy32_wbf_dx32", (F32, BF16, F32))),
    "wgrad": (("f32", (F32, F32)), ("x16_dybf", (F16, BF16)), ("x32_dybf", (F32, BF16)), ("x16_dy32", (F16, F32))),
}
# the stored residual sum of the addrelu form: fp32, or fp16 (one rounding of the exact fp32 value)
SUM_TYPES = (F32, F16)


def arith_type(mode, direction):
    """T of the matrix instruction (dj_launch_lowp_io): fp16 for the forward GEMM of mode float16, bf16 otherwise."""
    assert mode in MODES
    return F16 if (mode == "float16" and direction == "fwd") else BF16


def model_round(t, dt):
    """Round-to-nearest-even to fp16 / bf16 and back, by torch's own conversion; -> fp64.  `t` holds fp32 values."""
    if dt is None or dt == F32:
        return t.double()
    return t.to(F32).to(dt).double()


def truncate(t, dt):
    """Round toward zero instead (a perturbed model for the premise test): the low fp32 mantissa bits cleared -- 13 for
    fp16 (values in its normal range), 16 for bf16."""
    if dt is None or dt == F32:
        return t.double()
    bits = t.to(F32).contiguous().view(torch.int32)
    mask = -(1 << (13 if dt == F16 else 16))
    return (bits & mask).view(F32).double()


# ---- which kernel runs, what may be launched (restated from dj_conv_launch.h fast_mode and dj_conv.hip) ------------------
def out_size(g):
    from oracle import keras_ops as ko
    if g.pad == "same":
        return ko.same_padding(g.h, g.k, g.s, g.dil)[2], ko.same_padding(g.w, g.k, g.s, g.dil)[2]
    return ko.valid_out_size(g.h, g.k, g.s, g.dil), ko.valid_out_size(g.w, g.k, g.s, g.dil)


def pads(g):
    from oracle import keras_ops as ko
    if g.pad == "same":
        return ko.same_padding(g.h, g.k, g.s, g.dil)[0], ko.same_padding(g.w, g.k, g.s, g.dil)[0]
    return 0, 0


def is_scatter(g, bias=False):
    """dgrad_is_strided_1x1 and no bias: the input gradient runs as a compact GEMM whose rows are scattered."""
    return g.k == 1 and g.s > 1 and pads(g) == (0, 0) and not bias


def branch_free(g, direction, bias=False):
    """fast_mode<AM, BMD>(p) != 0 for dense, 16-byte aligned tensors: the 16-bit-tile kernel runs in modes 1 / 2."""
    if direction == "fwd":                        # <0, 0>: srcC = in_c, N = ldb = out_c
        return g.ci % 32 == 0 and g.co % 4 == 0
    if direction == "wgrad":                      # <2, 0>: srcC = in_c % 4, N = out_c, ldb = ld_y
        return g.ci % 4 == 0 and g.co % 4 == 0
    if is_scatter(g, bias):                       # <0, 1>: srcC = out_c
        return g.co % 32 == 0
    return g.co % 32 == 0 and g.s == 1            # <1, 1>: srcC = out_c, unit stride


def addrelu_supported(g):
    """dj_conv2d_fwd_addrelu_supported."""
    return g.k == 1 and g.s == 1 and pads(g) == (0, 0) and g.ci % 32 == 0 and g.co % 4 == 0


def form_applies(g, direction, form):
    if form == "addrelu_sum":
        return addrelu_supported(g)
    if form == "scatter":
        return is_scatter(g)
    if form in ("plain", "beta") and direction == "dgrad":
        return not is_scatter(g)
    if form in ("bnb_masked", "bnb_unmasked"):
        return not is_scatter(g)                  # "not for strided 1x1 convolutions (their dx is scattered)"
    return True


def any16(types):
    return any(t != F32 for t in types)


def legal(g, direction, form, types, mode):
    """May this launch be made?  False: it must raise DjError and write nothing.  16-bit tensors exist in mode float16
    only and need the branch-free kernel (include/dj_hip.h: storage-type codes)."""
    if not any16(types):
        return True
    return mode == "float16" and branch_free(g, direction, bias=(form == "transpose_bias"))


def cases(mode):
    """Every (geometry, direction, form, storage name, types, legal) of a mode.  The off-precondition geometries take
    16-bit tensors only to be refused: one form per direction is enough for that."""
    out = []
    for g in GEOMS:
        for direction, forms in FORMS.items():
            for form in forms:
                if not form_applies(g, direction, form):
                    continue
                for sname, types in STORAGE[direction]:
                    if form in ("slabs", "atomics") and types[2] != F32:
                        continue                  # a 16-bit result is written by one K range
                    ok = legal(g, direction, form, types, mode)
                    out.append((g, direction, form, sname, types, ok))
    return out


def split_k(K, splits):
    """dj_conv.hip split_k: K ranges that are not empty when `splits` are asked for (ranges are multiples of 32)."""
    chunk = -(-(-(-K // splits)) // 32) * 32
    return -(-K // chunk)


# ---- seeded operands ------------------------------------------------------------------------------------------------------
def _grid(shape, kmax, gen):
    return torch.randint(-kmax, kmax + 1, shape, generator=gen).to(F32) / 1024.0


def _scales(n, gen):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=gen)]


@functools.lru_cache(maxsize=None)
def operands(name):
    """fp32 host tensors of one geometry; computed once, never written to."""
    g = GEOM[name]
    gen = torch.Generator().manual_seed(1000 + [q.name for q in GEOMS].index(name))
    oh, ow = out_size(g)
    d = {}
    d["x"] = torch.randn(g.b, g.h, g.w, g.ci, generator=gen)                  # meets the kernel without a prologue
    d["xg"] = _grid((g.b, g.h, g.w, g.ci), 4096, gen)                         # goes through a prologue
    d["res"] = _grid((g.b, g.h, g.w, g.ci), 4096, gen)
    d["w"] = torch.randn(g.k, g.k, g.ci, g.co, generator=gen)
    d["dy"] = torch.randn(g.b, oh, ow, g.co, generator=gen) * 1e-3
    d["bias_co"] = torch.randn(g.co, generator=gen)
    d["bias_ci"] = torch.randn(g.ci, generator=gen) * 1e-3                    # of the transpose-forward use
    d["sc"], d["sh"] = _scales(g.ci, gen), _grid((g.ci,), 512, gen)
    d["rsc"], d["rsh"] = _scales(g.ci, gen), _grid((g.ci,), 512, gen)
    d["z"] = _grid((g.b, g.h, g.w, g.ci), 2048, gen)                          # |k| <= 2048: fp16 holds it exactly
    d["mean"], d["invstd"] = _grid((g.ci,), 512, gen), _scales(g.ci, gen)
    d["prev"] = torch.randn(g.b, g.h, g.w, g.ci, generator=gen) * 3e-2        # what a `beta` launch accumulates into
    return d


def stored(t, dt):
    """The tensor as it sits in HBM in storage type dt (pre-rounded: that rounding is part of the input, not the kernel)."""
    return t if dt == F32 else t.to(dt)


# ---- fp64 references ------------------------------------------------------------------------------------------------------
def pro_affine(x, sc, sh, relu=True):
    v = x.double() * sc.double() + sh.double()
    return torch.relu(v) if relu else v


def pro_addrelu(x, sc, sh, r, rsc, rsh):
    return torch.relu(x.double() * sc.double() + sh.double() + r.double() * rsc.double() + rsh.double())


def conv(g, a, w, bias=None):
    from oracle import keras_ops as ko
    return ko.conv2d(a, w, bias, (g.s, g.s), g.pad, (g.dil, g.dil))


def conv_dx(g, dy, w):
    x0 = torch.zeros(g.b, g.h, g.w, g.ci, dtype=torch.float64, requires_grad=True)
    conv(g, x0, w).backward(dy)
    return x0.grad


def conv_dw(g, a, dy):
    w0 = torch.zeros(g.k, g.k, g.ci, g.co, dtype=torch.float64, requires_grad=True)
    conv(g, a, w0).backward(dy)
    return w0.grad


def gemm_model(g, direction, a, b, T, rnd_a=model_round, rnd_b=model_round):
    """-> (model, sum|a||b|, K) of one GEMM: `a` the gathered operand AFTER its prologue (x, or dy), `b` the other one
    (w, or dy for the weight gradient), both holding fp32 values; T None: the unrounded oracle."""
    ar, br = rnd_a(a, T), rnd_b(b, T)
    op = {"fwd": conv, "dgrad": conv_dx, "wgrad": conv_dw}[direction]
    K = {"fwd": g.k * g.k * g.ci, "dgrad": g.k * g.k * g.co, "wgrad": g.b * out_size(g)[0] * out_size(g)[1]}[direction]
    return op(g, ar, br), op(g, ar.abs(), br.abs()), K


def elem_bound(S, K, adds=0, result=None):
    """(K + 2) u sum|a||b| + adds * u |result|."""
    bnd = (K + 2) * U * S
    return bnd + adds * U * result.abs() if adds else bnd


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def interval16(lo, hi, dt):
    """The 16-bit values a monotone RNE rounding can give for an fp32 value in [lo, hi] (fp64 tensors): torch rounds
    fp64 -> fp32 -> dt, each step monotone and the identity on the fp32 value itself.  -> (lowest, highest) as fp64."""
    return lo.to(F32).to(dt).double(), hi.to(F32).to(dt).double()


def stats_model(y, S, K):
    """Column totals of the forward statistics epilogue over the rows of the UNROUNDED result y [rows, C] (fp64, without
    bias) -> (sum, bound), (sum of squares, bound).  sum: u [(K + 2) sum_rows S + rows sum_rows |y|] -- every y carries
    its accumulation error, a fp32 sum of `rows` terms rows * u of their absolute sum.  Squares: twice that, relative:
    every row's term weighted by |y| (d(y^2) = 2 |y| dy; one rounding of the square, inside the doubled second term)."""
    rows = y.shape[0]
    b1 = U * ((K + 2) * S.sum(0) + rows * y.abs().sum(0))
    b2 = 2 * U * ((K + 2) * (S * y.abs()).sum(0) + rows * (y * y).sum(0))
    return (y.sum(0), b1), ((y * y).sum(0), b2)


def weighted_sum_model(y, S, K, weight, product_rounds):
    """Column totals of the BatchNormalization-backward epilogue: sum_rows y * weight with `weight` [rows, C] exact (the
    ReLU mask, or mask * x-hat on grid data) -> (total, bound); product_rounds: the product is rounded (x-hat), one more
    u per term."""
    rows = y.shape[0]
    t = y * weight
    return t.sum(0), U * ((K + 2) * (S * weight.abs()).sum(0) + (rows + (1 if product_rounds else 0)) * t.abs().sum(0))


# ---- the model per launch form --------------------------------------------------------------------------------------------
PERTURBATIONS = ("truncate", "b_unrounded", "swap", "pro_after", "stats_rounded")
Ref = collections.namedtuple("Ref", "pre S K adds relu result extra")
# pre: the fp64 model of the fp32 value the epilogue holds before ReLU and the store; S: sum|a||b| of its GEMM; adds: fp32
# additions behind the accumulation (bias, beta; a split reduction adds its own on top); result: relu(pre) if relu else
# pre; extra: {"sum": stored residual sum, "y": GEMM result without bias [rows, C], "S2": S as [rows, C], ...}


def _rounders(T, variant):
    if variant == "swap" and T is not None:
        T = BF16 if T == F16 else F16
    rnd = truncate if variant == "truncate" else model_round
    rnd_b = (lambda t, dt: t.double()) if variant == "b_unrounded" else rnd
    return T, rnd, rnd_b


def forward_ref(name, mode, form, types, variant=None):
    g, o = GEOM[name], operands(name)
    x_dt = types[0]
    T, rnd, rnd_b = _rounders(arith_type(mode, "fwd") if branch_free(g, "fwd") else None, variant)
    extra, bias, relu = {}, None, False
    if form == "plain_bias_relu":
        a, bias, relu = stored(o["x"], x_dt).double(), o["bias_co"].double(), True
    else:
        xs = stored(o["xg"], x_dt)
        if form == "addrelu_sum":
            pro = lambda t: pro_addrelu(t, o["sc"], o["sh"], stored(o["res"], x_dt), o["rsc"], o["rsh"])
        else:
            pro = lambda t: pro_affine(t, o["sc"], o["sh"], True)
        if variant == "pro_after" and T is not None:          # rounds x, then runs the prologue: the wrong order
            a, rnd = pro(rnd(xs, T)), (lambda t, dt: t.double())
        else:
            a = pro(xs)
        if form == "addrelu_sum":
            extra["sum"] = a
    y, S, K = gemm_model(g, "fwd", a, o["w"], T, rnd, rnd_b)
    extra["y"], extra["S2"] = y.reshape(-1, g.co), S.reshape(-1, g.co)
    pre = y + bias if bias is not None else y
    return Ref(pre, S, K, 1 if bias is not None else 0, relu, torch.relu(pre) if relu else pre, extra)


def dgrad_ref(name, mode, form, types, variant=None):
    g, o = GEOM[name], operands(name)
    dy_dt, dx_dt = types[0], types[2]
    with_bias = form == "transpose_bias"
    T, rnd, rnd_b = _rounders(BF16 if branch_free(g, "dgrad", with_bias) else None, variant)
    y, S, K = gemm_model(g, "dgrad", stored(o["dy"], dy_dt).double(), o["w"], T, rnd, rnd_b)
    extra = {"y": y.reshape(-1, g.ci), "S2": S.reshape(-1, g.ci)}
    pre, adds = y, 0
    if with_bias:
        pre, adds = y + o["bias_ci"].double(), 1
    if form == "beta":
        pre, adds = y + stored(o["prev"], dx_dt).double(), 1
    if form in ("bnb_masked", "bnb_unmasked"):
        z = stored(o["z"], F16).double().reshape(-1, g.ci)
        mask = (z * o["sc"].double() + o["sh"].double() > 0).double() if form == "bnb_masked" else torch.ones_like(z)
        extra["mask"], extra["xhat"] = mask, mask * (z - o["mean"].double()) * o["invstd"].double()
    return Ref(pre, S, K, adds, False, pre, extra)


def wgrad_ref(name, mode, form, types, variant=None):
    g, o = GEOM[name], operands(name)
    x_dt, dy_dt = types
    T, rnd, rnd_b = _rounders(BF16 if branch_free(g, "wgrad") else None, variant)
    if form == "plain":
        a = stored(o["x"], x_dt).double()
    elif variant == "pro_after" and T is not None:
        a, rnd = pro_affine(rnd(stored(o["xg"], x_dt), T), o["sc"], o["sh"], True), (lambda t, dt: t.double())
    else:
        a = pro_affine(stored(o["xg"], x_dt), o["sc"], o["sh"], True)
    y, S, K = gemm_model(g, "wgrad", a, stored(o["dy"], dy_dt).double(), T, rnd, rnd_b)
    return Ref(y, S, K, 0, False, y, {})


REFS = {"fwd": forward_ref, "dgrad": dgrad_ref, "wgrad": wgrad_ref}


# ---- the assertions, on whatever device the tensors live --------------------------------------------------------------------
def check_f32(got, ref, extra_adds=0):
    """fp32 result -> (rel-L2 to the model, largest |got - model| / bound); NaN anywhere gives (nan, nan)."""
    got, model, pre = got.double(), ref.result.to(got.device), ref.pre.to(got.device)
    bound = elem_bound(ref.S.to(got.device), ref.K, ref.adds + extra_adds, pre)
    err = (got - model).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    return rel_l2(got, model), ratio


def passes_f32(rel, ratio):
    return rel <= REL_L2_BOUND and ratio <= 1.0        # (both False for NaN)


def check_16(got, ref, dt):
    """16-bit result -> number of elements outside [round(lo), round(hi)], lo / hi = the ends of the fp32 interval the
    per-element bound allows: equal to model_round(model) wherever the interval holds no rounding boundary, else that
    value or its neighbour on the other side of the boundary."""
    assert got.dtype == dt
    dev = got.device
    pre = ref.pre.to(dev)
    bound = elem_bound(ref.S.to(dev), ref.K, ref.adds, pre)
    lo, hi = pre - bound, pre + bound
    if ref.relu:
        lo, hi = torch.relu(lo), torch.relu(hi)
    lo16, hi16 = interval16(lo, hi, dt)
    g = got.double()
    inside = (g >= lo16) & (g <= hi16)
    return int((~inside).sum()), int((lo16 != hi16).sum())
