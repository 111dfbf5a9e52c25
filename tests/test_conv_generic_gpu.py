"""The generic implicit-GEMM kernel (dj_igemm_kernel, csrc/dj_igemm.h) at every variant a tuning entry can name for it: the
four tile shapes x split-K by atomics and through slabs, the scalar and vector paths of both operands in every GEMM role,
the K tail, a K-step that spans several taps, the strided-1x1 scatter, and the statistics / BatchNormalization-backward /
masked epilogues on full and on edge tiles.  It is what runs the 126-filter predictor heads, the RGB stem, every strided
non-1x1 input gradient and any unaligned channel slice; engine.Plan.autotune may register any tile index times a split
factor for those launches.  Cases and what each is the smallest instance of: tests/conv_geometry_cases.py (the CPU test
beside it shows that together they reach every path).

Every output lies in a NaN-filled buffer with guard columns on both sides and a guard image before and after it, and the
guards must still be NaN afterwards: a write outside the tensor fails the test instead of landing in the allocator's slack.
Inputs that are views have NaN around them as well: a read outside them poisons the result.

Routing: each clause of fast_mode<AM, BMD> (csrc/dj_conv_launch.h) decides whether a launch goes to kernels that load 16
bytes at a time without guards.  In arithmetic mode float16 with fp32 tensors a minimally ineligible geometry must come out
at the fp32 bound (it ran the generic fp32 kernel) and its eligible twin above 1e-5 (the reduced-precision kernel ran)."""
import functools

import pytest
import torch

import conv_geometry_cases as cg

pytestmark = pytest.mark.gpu

NAN = float("nan")
SPLITS = (1, 2, 3)
ALIASES = ((9, 0), (cg.N_CFG + 2, 2))       # (configuration index, the tile index it names on the generic kernel)
IDS = cg.case_id


@pytest.fixture()
def lib():
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    handle = _lib.load()
    yield handle
    handle.dj_set_fast_path(1)
    handle.dj_set_gather_variants(1)
    K.set_floatx("float32")


def _tol(ref):
    return 1e-3 * float(ref.abs().max()) + 1e-5


def close(got, ref):
    """rel-L2 <= 2e-6 against fp64 and the max-norm bound of tests/test_conv_gpu.py -> (ok, figures)."""
    got = got.double()
    e2 = float((got - ref).norm() / ref.norm())
    emax = float((got - ref).abs().max())
    return e2 <= 2e-6 and emax <= _tol(ref), (e2, emax)


class Guarded(object):
    """An NHWC tensor `t` inside a NaN-filled buffer: a guard image before and after it, guard columns on both sides."""

    def __init__(self, shape, view67=False, fill=None):
        b, h, w, c = shape
        if view67:
            assert c == 64
            self.buf = torch.full((b + 2, h, w, 67), NAN, device="cuda")
            self.t = self.buf[1:b + 1, :, :, 1:65]
        else:
            self.buf = torch.full((b + 2, h, w, c + 8), NAN, device="cuda")
            self.t = self.buf[1:b + 1, :, :, 4:4 + c]
        self.inside = torch.zeros_like(self.buf, dtype=torch.bool)
        self.inside[1:b + 1, :, :, (1 if view67 else 4):(65 if view67 else 4 + c)] = True
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[~self.inside]).all())


class GuardedFlat(object):
    """A contiguous tensor (weight gradient, statistics rows) with 64 NaN floats before and after it."""

    def __init__(self, shape, fill=NAN):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 128,), NAN, device="cuda")
        self.t = self.buf[64:64 + n].view(shape)
        self.t.fill_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[:64]).all() and torch.isnan(self.buf[-64:]).all())


def view_input(t, kind):
    """The input tensor `t` (cuda) as the case's layout holds it, NaN around it."""
    if kind == "view67":
        buf = torch.full(t.shape[:3] + (67,), NAN, device="cuda")
        buf[..., 1:65] = t
        return buf[..., 1:65]
    return t


def offset_weights(w, byte_off):
    """The weights `byte_off` bytes past a 16-byte boundary, contiguous, NaN around them."""
    if not byte_off:
        return w
    assert byte_off % 4 == 0
    flat = torch.full((w.numel() + 8,), NAN, device="cuda")
    v = flat[byte_off // 4:byte_off // 4 + w.numel()].view(w.shape)
    v.copy_(w)
    assert v.is_contiguous() and v.data_ptr() % 16 == byte_off
    return v


@functools.lru_cache(maxsize=None)
def device_case(case_index):
    """Descriptor, device operands in the case's layout and the oracle's results on the device (fp64): made once, never
    written to."""
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    case = cg.GENERIC_KERNEL_CASES[case_index]
    b, h, w, ci, co, k, s, pad, d = cg.norm(case.geom)
    host, ref = cg.reference(case.geom)
    desc = Kn.make_conv_desc(b, h, w, ci, co, k, s, pad, d)
    kind = case.layout.name
    dev = {n: t.cuda() for n, t in host.items()}
    dev["x"], dev["dy"] = view_input(dev["x"], kind), view_input(dev["dy"], kind)
    dev["w"] = offset_weights(dev["w"], case.layout.off_w)
    assert dev["x"].data_ptr() % 16 == case.layout.off_x and dev["dy"].data_ptr() % 16 == case.layout.off_y
    assert Kn._pixel_ld(dev["x"]) == (case.layout.ld_x or ci) and Kn._pixel_ld(dev["dy"]) == (case.layout.ld_y or co)
    g = torch.Generator().manual_seed(5)
    dev["dx0"] = (torch.randn(b, h, w, ci, generator=g) * 1e-3).cuda()
    # a BatchNormalization in front of the convolution, for the input gradient that takes its backward statistics: z = x,
    # a mask z * bsc + bsh > 0 that cuts through every channel
    dev["mean"], dev["invstd"] = (torch.randn(ci, generator=g) * 0.3).cuda(), (torch.rand(ci, generator=g) + 0.5).cuda()
    dev["bsc"], dev["bsh"] = (torch.rand(ci, generator=g) + 0.5).cuda(), (torch.randn(ci, generator=g) * 0.5).cuda()
    dev["z"] = host["x"].cuda()
    rd = {n: t.cuda() for n, t in ref.items()}
    rd["y_bias_relu"] = torch.relu(rd["y"] + host["bias"].double().cuda())
    rd["y_pro_bias_relu"] = torch.relu(rd["y_pro"] + host["bias"].double().cuda())
    raw = rd["y_pro"].reshape(-1, co)
    rd["s"], rd["q"] = raw.sum(0), (raw * raw).sum(0)
    rd["dx_beta"] = rd["dx"] + dev["dx0"].double()
    rd["dx_mask"] = torch.where(dev["z"] > 0, rd["dx"], torch.zeros_like(rd["dx"]))
    return case, desc, dev, rd


def stats_ok(stats, rd):
    st = stats.double().sum(dim=0)
    return bool((st[0] - rd["s"]).abs().max() <= 1e-3 * rd["s"].abs().max() + 1e-3 and
                (st[1] - rd["q"]).abs().max() <= 1e-3 * rd["q"].abs().max())


@pytest.mark.parametrize("index", range(len(cg.GENERIC_KERNEL_CASES)), ids=lambda i: IDS(cg.GENERIC_KERNEL_CASES[i]))
def test_generic_kernel_every_tile_and_split(index, lib):
    from jpeg_detection_resnet_ssd_amd import _lib, engine
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    case, desc, dev, rd = device_case(index)
    b, h, w, ci, co, k, s, pad, d = cg.norm(case.geom)
    v67 = case.layout.name == "view67"
    x, wt, dy, sc, sh, bias = dev["x"], dev["w"], dev["dy"], dev["sc"], dev["sh"], dev["bias"]
    y_shape, x_shape = tuple(rd["y"].shape), (b, h, w, ci)
    rows_in = b * h * w
    scatter = case.route["dgrad"].startswith("scatter")
    dbias = (torch.randn(ci, generator=torch.Generator().manual_seed(9))).cuda()
    bad = []

    def generic_for(role):
        # a role whose launches would take the branch-free kernels runs with them switched off; for the others the launcher's
        # own routing is part of what is tested
        lib.dj_set_fast_path(0 if case.route[role] == "fast" else 1)
        assert cg.launch(role, case.geom, case.layout, allow_fast=case.route[role] != "fast").fast == 0

    def pin(direction, cfg, splits):
        _lib.check(lib.dj_conv2d_tune_set(direction, desc, cfg, splits), "tune_set")

    def expect(tag, got, ref_name, *guards):
        ok, figures = close(got, rd[ref_name])
        if not ok:
            bad.append((tag, ref_name, figures))
        for gd in guards:
            if not gd.intact():
                bad.append((tag, ref_name, "a guard element was written"))

    def fwd_bias_relu(cfg, splits):
        pin(0, cfg, splits)
        y = Guarded(y_shape, v67)
        Kn.conv2d_fwd(desc, x, wt, bias, y.t, relu=True)
        return y

    def dgrad_plain(cfg, splits):
        pin(1, cfg, splits)
        dx = Guarded(x_shape, v67)
        Kn.conv2d_dgrad(desc, dy, wt, dx.t)
        return dx

    def wgrad_plain(cfg, splits):
        pin(2, cfg, splits)
        dw = GuardedFlat(wt.shape, 7.0 if splits > 1 else NAN)      # (a split launch clears dw itself)
        Kn.conv2d_wgrad(desc, x, dy, dw.t)
        return dw

    try:
        kept = {}
        for tile in range(4):
            # ---------------- forward ----------------
            generic_for("fwd")
            for splits in SPLITS:
                tag = "fwd tile %d splits %d" % (tile, splits)
                # bias + ReLU; split: atomics onto the cleared slice, then the ReLU pass over the slice
                y = fwd_bias_relu(tile, splits)
                expect(tag, y.t, "y_bias_relu", y)
                if splits == 1:
                    kept["fwd", tile] = y.t.clone()
                # through slabs, statistics from the reduction: two launches, the same bits
                pin(0, tile, splits)
                need = Kn.conv2d_fwd_workspace_floats(desc, True)
                ws = torch.full((max(need, 4),), NAN, device="cuda")
                outs = []
                for _ in range(2):
                    y, st = Guarded(y_shape, v67), GuardedFlat((Kn.conv2d_stats_rows(desc), 2, co))
                    Kn.conv2d_fwd(desc, x, wt, bias, y.t, sc, sh, True, True, st.t, workspace=ws, stats_may_split=True)
                    outs.append((y, st))
                expect(tag + " slabs", outs[0][0].t, "y_pro_bias_relu", outs[0][0], outs[0][1])
                if not (torch.equal(outs[0][0].t, outs[1][0].t) and torch.equal(outs[0][1].t, outs[1][1].t)):
                    bad.append((tag, "two slab launches differ"))
                if not stats_ok(outs[0][1].t, rd):
                    bad.append((tag, "statistics of the slab reduction"))
                # a workspace that is too small: one K range after all (the statistics cannot come from atomics)
                y, st = Guarded(y_shape, v67), GuardedFlat((Kn.conv2d_stats_rows(desc), 2, co))
                Kn.conv2d_fwd(desc, x, wt, bias, y.t, sc, sh, True, True, st.t, workspace=torch.empty(8, device="cuda"),
                              stats_may_split=True)
                expect(tag + " small workspace", y.t, "y_pro_bias_relu", y, st)
                if not stats_ok(st.t, rd):
                    bad.append((tag, "statistics with a small workspace"))
            # prologue + bias + ReLU + statistics from the GEMM epilogue (one K range whatever is registered)
            pin(4, tile, 2)
            y, st = Guarded(y_shape, v67), GuardedFlat((Kn.conv2d_stats_rows(desc), 2, co))
            Kn.conv2d_fwd(desc, x, wt, bias, y.t, sc, sh, True, True, st.t)
            expect("fwd tile %d statistics" % tile, y.t, "y_pro_bias_relu", y, st)
            if not stats_ok(st.t, rd):
                bad.append(("fwd tile %d" % tile, "statistics of the epilogue"))

            # ---------------- input gradient ----------------
            generic_for("dgrad")
            for splits in SPLITS:
                tag = "dgrad tile %d splits %d" % (tile, splits)
                dx = dgrad_plain(tile, splits)
                expect(tag, dx.t, "dx", dx)
                if splits == 1:
                    kept["dgrad", tile] = dx.t.clone()
                dxb = Guarded(x_shape, v67, fill=dev["dx0"])
                Kn.conv2d_dgrad(desc, dy, wt, dxb.t, beta=True)
                expect(tag + " beta", dxb.t, "dx_beta", dxb)
                if scatter:      # the pixels between the strides: exactly zero, or exactly what was there
                    off = torch.ones(x_shape, dtype=torch.bool, device="cuda")
                    off[:, ::s[0], ::s[1], :] = False
                    if not (bool((dx.t[off] == 0).all()) and torch.equal(dxb.t[off], dev["dx0"][off])):
                        bad.append((tag, "pixels between the strides"))
            pin(1, tile, 2)
            dx = Guarded(x_shape, v67)
            Kn.conv2d_dgrad(desc, dy, wt, dx.t, bias=dbias, no_split=True)
            ok, figures = close(dx.t, rd["dx"] + dbias.double())
            if not ok or not dx.intact():
                bad.append(("dgrad tile %d bias, one K range" % tile, figures, dx.intact()))
            if not scatter:
                pin(1, tile, 1)
                dx = Guarded(x_shape, v67)
                Kn.conv2d_dgrad(desc, dy, wt, dx.t, relu_mask=dev["z"])
                expect("dgrad tile %d ReLU mask" % tile, dx.t, "dx_mask", dx)
                pin(1, tile, 2)                                           # (a registered split is overridden)
                for masked in (True, False):
                    tag = "dgrad tile %d BN backward statistics%s" % (tile, " masked" if masked else "")
                    dx, part = Guarded(x_shape, v67), GuardedFlat(((rows_in + 63) // 64, 2, ci))
                    Kn.conv2d_dgrad_bnbwd(desc, dy, wt, dx.t, dev["z"], dev["mean"], dev["invstd"],
                                          dev["bsc"] if masked else None, dev["bsh"] if masked else None, part.t)
                    expect(tag, dx.t, "dx", dx, part)
                    # column totals of the partial rows: against fp64 on the stored gradient, and against dj_bn_bwd_reduce
                    gm, z2 = dx.t.double().reshape(rows_in, ci), dev["z"].double().reshape(rows_in, ci)
                    if masked:
                        gm = torch.where(z2 * dev["bsc"].double() + dev["bsh"].double() > 0, gm, torch.zeros_like(gm))
                    want = (gm.sum(0), (gm * (z2 - dev["mean"].double()) * dev["invstd"].double()).sum(0))
                    dxc = dx.t.contiguous()
                    part2 = torch.empty(engine.query("dj_reduce_rows", rows_in), 2, ci, device="cuda")
                    engine.call("dj_bn_bwd_reduce", dxc, ci, dev["z"], ci, None, 0, dev["mean"], dev["invstd"], dev["bsc"],
                                dev["bsh"], 2 if masked else 0, rows_in, ci, part2)
                    got = part.t.double()
                    if not bool(torch.isfinite(got).all()):
                        bad.append((tag, "partial rows not finite"))
                    for slot in (0, 1):
                        lim = 1e-4 * float(want[slot].abs().max()) + 1e-3
                        e1 = float((got[:, slot].sum(0) - want[slot]).abs().max())
                        e2 = float((got[:, slot].sum(0) - part2.double()[:, slot].sum(0)).abs().max())
                        if not (e1 <= lim and e2 <= lim):
                            bad.append((tag, "slot %d" % slot, e1, e2, lim))

            # ---------------- weight gradient ----------------
            generic_for("wgrad")
            for splits in SPLITS:
                tag = "wgrad tile %d splits %d" % (tile, splits)
                dw = wgrad_plain(tile, splits)
                expect(tag, dw.t, "dw", dw)
                if splits == 1:
                    kept["wgrad", tile] = dw.t.clone()
                dw = GuardedFlat(wt.shape, 0.0)
                Kn.conv2d_wgrad(desc, x, dy, dw.t, sc, sh, True, dw_zeroed=True)
                expect(tag + " prologue, zeroed", dw.t, "dw_pro", dw)
            pin(2, tile, 1)
            dw = GuardedFlat(wt.shape)
            Kn.conv2d_wgrad(desc, x, dy, dw.t, sc, sh, True)
            expect("wgrad tile %d prologue" % tile, dw.t, "dw_pro", dw)

        # the other indices name the same four instantiations on this kernel: with one K range, the same bits
        for cfg, tile in ALIASES:
            assert cg.GENERIC_TILE_OF_CFG[cfg % cg.N_CFG] == tile
            for role, run in (("fwd", fwd_bias_relu), ("dgrad", dgrad_plain), ("wgrad", wgrad_plain)):
                generic_for(role)
                if not torch.equal(run(cfg, 1).t, kept[role, tile]):
                    bad.append(("configuration %d is not tile %d" % (cfg, tile), role))
        torch.cuda.synchronize()
        assert not bad, bad[:12]
    finally:
        lib.dj_set_fast_path(1)
        for direction in (0, 4, 1, 2):
            _lib.check(lib.dj_conv2d_tune_set(direction, desc, -1, 1), "tune_set")


# (clause of fast_mode, role, ineligible geometry, its x layout (ld, channel offset) or None, eligible twin, its x layout)
BASE = (2, 6, 7, 64, 64, 3, 1, "same", 1)
ROUTING = [
    ("Cin % 32", "fwd", (2, 6, 7, 48, 64, 3, 1, "same", 1), None, BASE, None),
    ("N % 4", "fwd", (2, 6, 7, 64, 62, 3, 1, "same", 1), None, BASE, None),
    ("input-gradient stride", "dgrad", (2, 6, 7, 64, 64, 3, 2, "same", 1), None, BASE, None),
    ("Cout % 32 of the input gradient", "dgrad", (2, 6, 7, 64, 48, 3, 1, "same", 1), None, BASE, None),
    ("Cin % 4 of the weight gradient", "wgrad", (2, 6, 7, 62, 64, 3, 1, "same", 1), None, BASE, None),
    ("ld % 4", "fwd", BASE, (65, 0), BASE, (68, 0)),
    ("pointer alignment", "fwd", BASE, (68, 1), BASE, (68, 4)),
]


def _run_role(role, geom, xlayout):
    """One launch of `role` at the launcher's default choice -> rel-L2 against the fp64 oracle."""
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    b, h, w, ci, co, k, s, pad, d = cg.norm(geom)
    host, ref = cg.reference(geom)
    desc = Kn.make_conv_desc(b, h, w, ci, co, k, s, pad, d)
    x = host["x"].cuda()
    if xlayout is not None:
        ld, off = xlayout
        buf = torch.full((b, h, w, ld), NAN, device="cuda")
        buf[..., off:off + ci] = x
        x = buf[..., off:off + ci]
        assert cg.route(role, geom, cg.Layout("x", ld, 4 * off, None, 0, 0)) == ("fast" if (ld % 4 == 0 and off % 4 == 0)
                                                                                  else "generic:sv")
    wt, dy = host["w"].cuda(), host["dy"].cuda()
    if role == "fwd":
        out, name = Kn.conv2d_fwd(desc, x, wt, None, torch.full(tuple(ref["y"].shape), NAN, device="cuda")), "y"
    elif role == "dgrad":
        out, name = Kn.conv2d_dgrad(desc, dy, wt, torch.full((b, h, w, ci), NAN, device="cuda")), "dx"
    else:
        out, name = Kn.conv2d_wgrad(desc, x, dy, torch.full(tuple(wt.shape), NAN, device="cuda")), "dw"
    torch.cuda.synchronize()
    return cg.rel_l2(out.cpu(), ref[name])


@pytest.mark.parametrize("clause,role,geom,xlayout,twin,twin_layout", ROUTING, ids=[r[0] for r in ROUTING])
def test_each_clause_of_the_routing_keeps_a_launch_off_the_branch_free_kernels(clause, role, geom, xlayout, twin, twin_layout,
                                                                               lib):
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    if xlayout is None:
        assert cg.route(role, geom).startswith("generic") and cg.route(role, twin) == "fast"
    K.set_floatx("float16")
    e_generic, e_twin = _run_role(role, geom, xlayout), _run_role(role, twin, twin_layout)
    K.set_floatx("float32")
    # 2e-6: the fp32 bound -- the generic fp32 kernel ran; 1e-5: the floor tests/test_lowp_gpu.py asserts for "the
    # reduced-precision kernel did run" (operand rounding: 1e-4 .. 1e-2)
    assert e_generic <= 2e-6, (clause, e_generic)
    assert 1e-5 < e_twin <= 8e-3, (clause, e_twin)


def test_16_bit_tensors_on_an_ineligible_geometry_are_refused_before_anything_is_written(lib):
    from jpeg_detection_resnet_ssd_amd import _lib
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    K.set_floatx("float16")
    F16, BF16 = torch.float16, torch.bfloat16

    def operands(geom):
        b, h, w, ci, co, k, s, pad, d = cg.norm(geom)
        host, ref = cg.reference(geom)
        return (Kn.make_conv_desc(b, h, w, ci, co, k, s, pad, d), host["x"].cuda(), host["w"].cuda(), host["dy"].cuda(),
                tuple(ref["y"].shape), (b, h, w, ci))

    # forward, Cin % 32 != 0
    desc, x, wt, dy, y_shape, x_shape = operands(ROUTING[0][2])
    y = torch.full(y_shape, NAN, device="cuda")
    with pytest.raises(_lib.DjError, match="16-bit"):
        Kn.conv2d_fwd(desc, x.to(F16), wt, None, y)
    # a split launch clears its output first: the refusal comes before that as well
    _lib.check(lib.dj_conv2d_tune_set(0, desc, 0, 3), "tune_set")
    try:
        with pytest.raises(_lib.DjError, match="16-bit"):
            Kn.conv2d_fwd(desc, x.to(F16), wt, None, y)
    finally:
        _lib.check(lib.dj_conv2d_tune_set(0, desc, -1, 1), "tune_set")
    # input gradient, stride 2; and the strided-1x1 scatter form with Cout % 32 != 0, which clears dx before it launches
    desc2, _, wt2, dy2, _, x_shape2 = operands(ROUTING[2][2])
    dx2 = torch.full(x_shape2, NAN, device="cuda")
    with pytest.raises(_lib.DjError, match="16-bit"):
        Kn.conv2d_dgrad(desc2, dy2.to(BF16), wt2, dx2)
    desc3, _, wt3, dy3, _, x_shape3 = operands((2, 8, 8, 64, 24, 1, 2, "valid", 1))
    dx3 = torch.full(x_shape3, NAN, device="cuda")
    with pytest.raises(_lib.DjError, match="16-bit"):
        Kn.conv2d_dgrad(desc3, dy3.to(BF16), wt3, dx3)
    # weight gradient, Cin % 4 != 0
    desc4, x4, wt4, dy4, _, _ = operands(ROUTING[4][2])
    dw4 = torch.full(tuple(wt4.shape), NAN, device="cuda")
    _lib.check(lib.dj_conv2d_tune_set(2, desc4, 0, 3), "tune_set")
    try:
        with pytest.raises(_lib.DjError, match="16-bit"):
            Kn.conv2d_wgrad(desc4, x4.to(F16), dy4.to(BF16), dw4)
    finally:
        _lib.check(lib.dj_conv2d_tune_set(2, desc4, -1, 1), "tune_set")
    torch.cuda.synchronize()
    for t in (y, dx2, dx3, dw4):
        assert bool(torch.isnan(t).all())
