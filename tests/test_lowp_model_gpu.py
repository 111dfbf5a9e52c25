"""The 16-bit-tile convolution GEMMs (csrc/dj_igemm_h16.h, PREC 1 / 2: K.set_floatx('float16' / 'bfloat16')) against their
exact operand-rounding model -- the fp64 convolution of the operands rounded where the kernel rounds them
(tests/lowp_model_cases.py; premises: tests/test_lowp_model_cpu.py) -- instead of the unrounded oracle at the size of
the rounding itself.  Every tuner index, splits 1 and 2 (weight gradient 1 / 2 / 3), every launch form, fp32 tensors and
every legal 16-bit storage combination, weight shadows 16- and 8-byte aligned, on the edge geometries of the cases file.

Results are views (pixel stride = channels + 16, 8 elements into the pixel) of NaN-filled buffers; what surrounds the view
is compared bit for bit.  (dw, the statistics rows and the partial sums have no stride in the C ABI: dw is a slice of a
NaN-filled flat buffer, guards on both sides.)

Assertions: fp32 results rel-L2 <= 2e-6 and per element |got - model| <= (K + 2) u sum|a||b| (+ u |result| per addition
behind the GEMM: bias, beta, each further K range of a split launch); 16-bit results inside [round(lo), round(hi)] of that
interval, i.e. equal to the rounded model wherever the interval holds no rounding boundary; the stored residual sum equal;
statistics and partial sums: fp64 column totals within u [(K + 2) sum_rows S + rows sum_rows |y|] of those of the UNROUNDED
result (squares: twice that, relative) and -- because that rigorous bound is far wider than one 16-bit rounding of y
averaged over a column (test_lowp_model_cpu.py, test_statistics_of_the_rounded_result_are_told_apart) -- within 2e-6
rel-L2 over the columns, squares 4e-6: a total of results that are each that close to the model.  The off-precondition
geometry equals the UNROUNDED oracle; what may not be launched raises DjError before anything is written."""
import functools

import pytest
import torch

import lowp_model_cases as C
from lowp_model_cases import BF16, F16, F32

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD, OFF = 16, 8            # a result's pixel stride is channels + PAD; the view starts OFF elements into the pixel
MEASURED = {}               # (mode, direction) -> [largest rel-L2, largest ratio to the per-element bound]


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def make_out(shape, dt, zero=False, fill=None):
    """-> (NaN-filled buffer, the view a result is written to)."""
    c = shape[-1]
    buf = torch.full(tuple(shape[:-1]) + (c + PAD,), NAN, dtype=dt, device="cuda")
    view = buf[..., OFF:OFF + c]
    if zero:
        view.zero_()
    if fill is not None:
        view.copy_(fill)
    return buf, view


def surroundings_untouched(buf, c):
    pat = int(_bits(torch.full((1,), NAN, dtype=buf.dtype))[0])
    b = _bits(buf)
    return bool((b[..., :OFF] == pat).all()) and bool((b[..., OFF + c:] == pat).all())


def all_nan_bits(buf):
    pat = int(_bits(torch.full((1,), NAN, dtype=buf.dtype))[0])
    return bool((_bits(buf) == pat).all())


def make_flat_out(shape, fill):
    """A contiguous result (dw) as a slice of a NaN-filled flat buffer."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 32,), NAN, device="cuda")
    out = flat[16:16 + n].view(shape)
    out.fill_(fill)
    return flat, out


@functools.lru_cache(maxsize=None)
def device_operands(name):
    """Every operand of a geometry in every storage type it is read in; computed once, never written to."""
    from jpeg_detection_resnet_ssd_amd.engine import call
    g, o = C.GEOM[name], C.operands(name)
    d = {}
    for key, types in (("x", (F32, F16)), ("xg", (F32, F16)), ("res", (F32, F16)), ("dy", (F32, BF16)), ("z", (F32, F16)),
                       ("prev", (F32, BF16))):
        for dt in types:
            d[key, dt] = C.stored(o[key], dt).cuda()
    for key in ("bias_co", "bias_ci", "sc", "sh", "rsc", "rsh", "mean", "invstd"):
        d[key] = o[key].cuda()
    w = o["w"]
    n = w.numel()
    d["w", F32, False] = d["w", F32, True] = w.cuda()
    if n % 8 == 0:
        # two copies of the master weights in one flat buffer: 8 bytes and 16 bytes into their 16-bit shadows
        flat = torch.zeros(2 * n + 16, device="cuda")
        flat[4:4 + n] = w.reshape(-1).cuda()
        flat[n + 8:2 * n + 8] = w.reshape(-1).cuda()
        f16 = torch.zeros(2 * n + 16, dtype=F16, device="cuda")
        fbf = torch.zeros(2 * n + 16, dtype=BF16, device="cuda")
        call("dj_shadow_weights", flat, f16, fbf, 2 * n + 16)
        torch.cuda.synchronize()
        for dt, sh in ((F16, f16), (BF16, fbf)):
            d["w", dt, True] = sh[4:4 + n].view(w.shape)             # "@8"
            d["w", dt, False] = sh[n + 8:2 * n + 8].view(w.shape)
            assert d["w", dt, True].data_ptr() % 16 == 8 and d["w", dt, False].data_ptr() % 16 == 0
            for k8 in (True, False):
                assert torch.equal(d["w", dt, k8].cpu(), w.to(dt)), "dj_shadow_weights is not RNE"
    else:                                             # (off the preconditions: only ever refused)
        for dt in (F16, BF16):
            d["w", dt, True] = d["w", dt, False] = w.to(dt).cuda()
    return d


@functools.lru_cache(maxsize=None)
def device_ref(name, mode, direction, form, types):
    r = C.REFS[direction](name, mode, form, types)
    cu = lambda t: t.cuda() if torch.is_tensor(t) else t
    return C.Ref(cu(r.pre), cu(r.S), r.K, r.adds, r.relu, cu(r.result), {k: cu(v) for k, v in r.extra.items()})


def desc_of(g):
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    return Kn.make_conv_desc(g.b, g.h, g.w, g.ci, g.co, (g.k, g.k), (g.s, g.s), g.pad, (g.dil, g.dil))


def launch(name, mode, direction, form, sname, types, sum_dt=F32, record=None):
    """One launch of a form -> {"out": (buffer, view), ...}; the references are looked up by the same key.
    record (a list): every result buffer is appended to it and handed to the launch all NaN -- for launches that must be
    refused before anything is written."""
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    g, D, desc = C.GEOM[name], device_operands(name), desc_of(C.GEOM[name])
    oh, ow = C.out_size(g)
    k8 = "@8" in sname
    r = {}

    def out_view(shape, dt, zero=False, fill=None):
        pair = make_out(shape, dt, zero, fill) if record is None else make_out(shape, dt)
        if record is not None:
            record.append(pair[0])
        return pair

    def out_flat(shape, fill):
        pair = make_flat_out(shape, fill if record is None else NAN)
        if record is not None:
            record.append(pair[0])
        return pair

    if direction == "fwd":
        x_dt, w_dt, y_dt = types
        w = D["w", w_dt, k8]
        r["out"] = ybuf, y = out_view((g.b, oh, ow, g.co), y_dt, zero=(form == "atomics"))
        xg = D["xg", x_dt]
        if form == "plain_bias_relu":
            Kn.conv2d_fwd(desc, D["x", x_dt], w, D["bias_co"], y, relu=True)
        elif form == "bn_stats":
            r["stats"] = torch.zeros(Kn.conv2d_stats_rows(desc), 2, g.co, device="cuda")
            Kn.conv2d_fwd(desc, xg, w, None, y, D["sc"], D["sh"], True, False, r["stats"])
        elif form == "slabs":
            ws = torch.empty(2 * g.b * oh * ow * g.co, device="cuda")
            Kn.conv2d_fwd(desc, xg, w, None, y, D["sc"], D["sh"], True, False, None, workspace=ws)
        elif form == "atomics":
            Kn.conv2d_fwd(desc, xg, w, None, y, D["sc"], D["sh"], True, False, None, y_zeroed=True)
        else:
            r["sum"] = smbuf, sm = out_view((g.b, g.h, g.w, g.ci), sum_dt)
            Kn.conv2d_fwd_addrelu(desc, xg, w, None, y, D["sc"], D["sh"], D["res", x_dt], D["rsc"], D["rsh"], sm)
    elif direction == "dgrad":
        dy_dt, w_dt, dx_dt = types
        dy, w = D["dy", dy_dt], D["w", w_dt, k8]
        r["out"] = dxbuf, dx = out_view((g.b, g.h, g.w, g.ci), dx_dt, fill=D["prev", dx_dt] if form == "beta" else None)
        if form in ("plain", "scatter"):
            Kn.conv2d_dgrad(desc, dy, w, dx)
        elif form == "beta":
            Kn.conv2d_dgrad(desc, dy, w, dx, None, True)
        elif form == "transpose_bias":
            Kn.conv2d_dgrad(desc, dy, w, dx, D["bias_ci"], False, no_split=True)
        else:
            # z as fp16 wherever a 16-bit tensor may be launched at all (the grid values are the same in either type)
            z = D["z", F16 if (mode == "float16" and C.branch_free(g, "dgrad")) else F32]
            r["part"] = torch.zeros((g.b * g.h * g.w + 63) // 64, 2, g.ci, device="cuda")
            masked = form == "bnb_masked"
            Kn.conv2d_dgrad_bnbwd(desc, dy, w, dx, z, D["mean"], D["invstd"], D["sc"] if masked else None,
                                  D["sh"] if masked else None, r["part"])
    else:
        x_dt, dy_dt = types
        if form == "plain":
            r["flat"] = flat, dw = out_flat((g.k, g.k, g.ci, g.co), 7.0)       # the launcher clears dw when it splits
            Kn.conv2d_wgrad(desc, D["x", x_dt], D["dy", dy_dt], dw)
        else:
            r["flat"] = flat, dw = out_flat((g.k, g.k, g.ci, g.co), 0.0)
            Kn.conv2d_wgrad(desc, D["xg", x_dt], D["dy", dy_dt], dw, D["sc"], D["sh"], True, dw_zeroed=True)
    return r


def k_ranges(g, direction, form, types, splits):
    """K ranges the launch really runs (dj_conv.hip): statistics, one-K-range forms and 16-bit results are never split."""
    if direction == "fwd":
        if form == "bn_stats" or types[2] != F32:
            return 1
        return C.split_k(g.k * g.k * g.ci, splits)
    if direction == "dgrad":
        if form in ("scatter", "bnb_masked", "bnb_unmasked", "transpose_bias") or types[2] != F32:
            return 1
        return C.split_k(g.k * g.k * g.co, splits)
    return C.split_k(g.b * C.out_size(g)[0] * C.out_size(g)[1], splits)


def verify(name, mode, direction, form, sname, types, sum_dt, r, splits, tag):
    g = C.GEOM[name]
    ref = device_ref(name, mode, direction, form, types)
    key = MEASURED.setdefault((mode, direction), [0.0, 0.0])
    if direction == "wgrad":
        flat, got = r["flat"]
        assert all_nan_bits(flat[:16]) and all_nan_bits(flat[16 + got.numel():]), tag
        out_dt = F32
    else:
        buf, got = r["out"]
        out_dt = types[2]
        assert surroundings_untouched(buf, got.shape[-1]), tag
    if out_dt == F32:
        rel, ratio = C.check_f32(got, ref, extra_adds=k_ranges(g, direction, form, types, splits) - 1)
        key[0], key[1] = max(key[0], rel), max(key[1], ratio)
        assert C.passes_f32(rel, ratio), (tag, "rel-L2 %.3e, ratio to the bound %.3f" % (rel, ratio))
    else:
        bad, straddle = C.check_16(got, ref, out_dt)
        assert bad == 0, (tag, "%d elements off the rounded model (%d intervals hold a boundary)" % (bad, straddle))
    if "sum" in r:
        smbuf, sm = r["sum"]
        assert surroundings_untouched(smbuf, g.ci), tag
        assert torch.equal(sm.double(), C.model_round(ref.extra["sum"].float(), sum_dt)), (tag, "stored residual sum")
    if "stats" in r:
        (s1, b1), (s2, b2) = C.stats_model(ref.extra["y"], ref.extra["S2"], ref.K)
        st = r["stats"].double().sum(0)
        assert bool(((st[0] - s1).abs() <= b1).all()) and bool(((st[1] - s2).abs() <= b2).all()), (tag, "statistics")
        e1, e2 = C.rel_l2(st[0], s1), C.rel_l2(st[1], s2)
        assert e1 <= C.REL_L2_BOUND and e2 <= 2 * C.REL_L2_BOUND, (tag, "statistics rel-L2 %.3e %.3e" % (e1, e2))
    if "part" in r:
        pt = r["part"].double().sum(0)
        for i, (wname, rounds) in enumerate((("mask", False), ("xhat", True))):
            tot, bnd = C.weighted_sum_model(ref.extra["y"], ref.extra["S2"], ref.K, ref.extra[wname], rounds)
            assert bool(((pt[i] - tot).abs() <= bnd).all()), (tag, "partial sums", wname)
            e = C.rel_l2(pt[i], tot)
            assert e <= C.REL_L2_BOUND, (tag, "partial sums %s rel-L2 %.3e" % (wname, e))


TUNE_DIRS = {"fwd": (0, 4), "dgrad": (1, 9), "wgrad": (2,)}


@pytest.fixture()
def floatx():
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    yield K
    K.set_floatx("float32")


def sum_types(mode, form):
    return C.SUM_TYPES if (form == "addrelu_sum" and mode == "float16") else (F32,)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("direction", list(C.FORMS))
@pytest.mark.parametrize("name", [g.name for g in C.GEOMS])
def test_gemm_equals_its_rounding_model(name, direction, mode, floatx):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    g, desc = C.GEOM[name], desc_of(C.GEOM[name])
    todo = [c for c in C.cases(mode) if c[0].name == name and c[1] == direction and c[5]]
    assert todo
    floatx.set_floatx(mode)
    try:
        for cfg in range(lib.dj_conv2d_tune_configs()):
            for splits in ((1, 2, 3) if direction == "wgrad" else (1, 2)):
                for d in TUNE_DIRS[direction]:
                    _lib.check(lib.dj_conv2d_tune_set(d, desc, cfg, splits), "tune_set")
                done = []
                for _, _, form, sname, types, _ in todo:
                    if form in ("slabs", "atomics") and splits == 1:
                        continue                  # (without a split these are the plain launch)
                    for sum_dt in sum_types(mode, form):
                        r = launch(name, mode, direction, form, sname, types, sum_dt)
                        done.append((form, sname, types, sum_dt, r))
                torch.cuda.synchronize()
                for form, sname, types, sum_dt, r in done:
                    tag = "%s %s %s %s %s cfg %d splits %d" % (mode, name, direction, form, sname, cfg, splits)
                    verify(name, mode, direction, form, sname, types, sum_dt, r, splits, tag)
    finally:
        for d in TUNE_DIRS[direction]:
            _lib.check(lib.dj_conv2d_tune_set(d, desc, -1, 1), "tune_set")
        floatx.set_floatx("float32")
    print("\nlowp-model %s %s %s: so far largest rel-L2 %.3e, largest ratio to the per-element bound %.3f"
          % (mode, direction, name, *MEASURED.get((mode, direction), [0.0, 0.0])))


@pytest.mark.parametrize("mode", C.MODES)
def test_fallback_geometry_is_the_unrounded_oracle(mode, floatx):
    """Cin = 3, Cout = 126: the generic fp32 kernel runs in the 16-bit modes too -- within 2e-6 of the oracle on the
    UNROUNDED operands (the table's model for this geometry is that oracle; here it is restated without the table)."""
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    name = "fallback"
    g, o, D, desc = C.GEOM[name], C.operands(name), device_operands(name), desc_of(C.GEOM[name])
    oh, ow = C.out_size(g)
    floatx.set_floatx(mode)
    ybuf, y = make_out((g.b, oh, ow, g.co), F32)
    dxbuf, dx = make_out((g.b, g.h, g.w, g.ci), F32)
    flat, dw = make_flat_out((g.k, g.k, g.ci, g.co), 7.0)
    Kn.conv2d_fwd(desc, D["xg", F32], D["w", F32, False], None, y, D["sc"], D["sh"], True)
    Kn.conv2d_dgrad(desc, D["dy", F32], D["w", F32, False], dx)
    Kn.conv2d_wgrad(desc, D["x", F32], D["dy", F32], dw)
    torch.cuda.synchronize()
    a = C.pro_affine(o["xg"], o["sc"], o["sh"])
    want = (C.conv(g, a, o["w"].double()), C.conv_dx(g, o["dy"].double(), o["w"].double()), C.conv_dw(g, o["x"].double(), o["dy"].double()))
    errs = [C.rel_l2(t.cpu(), r) for t, r in zip((y, dx, dw), want)]
    assert max(errs) <= C.REL_L2_BOUND, errs
    assert surroundings_untouched(ybuf, g.co) and surroundings_untouched(dxbuf, g.ci)


@pytest.mark.parametrize("mode", C.MODES)
def test_illegal_combinations_raise_and_write_nothing(mode, floatx):
    """Every (geometry, form, storage) the table calls illegal -- 16-bit tensors off the branch-free preconditions, and
    any 16-bit tensor in mode bfloat16 -- with a split registered, so that a launcher that cleared its result before it
    refused would show."""
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    floatx.set_floatx(mode)
    todo = [c for c in C.cases(mode) if not c[5]]
    assert todo
    pinned = set()
    try:
        for g, direction, form, sname, types, _ in todo:
            if (g.name, direction) not in pinned:
                for d in TUNE_DIRS[direction]:
                    _lib.check(lib.dj_conv2d_tune_set(d, desc_of(g), 0, 2), "tune_set")
                pinned.add((g.name, direction))
            seen = []
            with pytest.raises(_lib.DjError):
                launch(g.name, mode, direction, form, sname, types, F16 if mode == "float16" else F32, record=seen)
            torch.cuda.synchronize()
            assert seen and all(all_nan_bits(b) for b in seen), (mode, g.name, direction, form, sname)
    finally:
        for name, direction in pinned:
            for d in TUNE_DIRS[direction]:
                _lib.check(lib.dj_conv2d_tune_set(d, desc_of(C.GEOM[name]), -1, 1), "tune_set")
        floatx.set_floatx("float32")
