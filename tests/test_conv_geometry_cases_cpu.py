"""What tests/test_conv_anisotropic_gpu.py and tests/test_conv_generic_gpu.py rely on, checked without a GPU: every case of
tests/conv_geometry_cases.py has the descriptor the oracle's output asks for, every anisotropic case is told apart from each
of its "one pair swapped between the axes" variants by the oracle, the restated launcher decisions send each case where its
comment says, and the generic cases together reach every path the generic kernel has."""
import pytest
import torch

import conv_geometry_cases as cg
from oracle import keras_ops as ko

ALL_CASES = cg.ANISOTROPIC + cg.GENERIC
IDS = cg.case_id


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_descriptor_has_the_oracle_output_size(case):
    from jpeg_detection_resnet_ssd_amd import kernels as Kn
    b, h, w, ci, co, k, s, pad, d = cg.norm(case.geom)
    host, ref = cg.reference(case.geom)
    desc = Kn.make_conv_desc(b, h, w, ci, co, k, s, pad, d)
    assert (desc.out_h, desc.out_w) == tuple(ref["y"].shape[1:3]) == cg.out_size(case.geom)
    (pt, _), (pl, _) = cg.explicit_pads(case.geom)
    assert (desc.pad_top, desc.pad_left) == (pt, pl)
    assert (desc.kernel_h, desc.kernel_w, desc.stride_h, desc.stride_w, desc.dilation_h, desc.dilation_w) == k + s + d
    # check_desc (csrc/dj_conv.hip): the last tap start lies inside the input
    assert (desc.out_h - 1) * desc.stride_h - desc.pad_top < h and (desc.out_w - 1) * desc.stride_w - desc.pad_left < w
    assert tuple(ref["dx"].shape) == (b, h, w, ci) and tuple(ref["dw"].shape) == k + (ci, co)
    # the prologue's shift hides nothing: it is above the data, positive somewhere (a padding pixel left at relu(shift) = 8
    # shows; with two dozen channels or more both signs occur), and the two references differ
    assert float(host["sh"].abs().min()) >= 8.0 > float((host["x"] * host["sc"]).abs().max())
    assert (host["sh"] > 0).any() and ((host["sh"] < 0).any() or ci < 24)
    assert cg.rel_l2(ref["y_pro"], ref["y"]) > 0.5


@pytest.mark.parametrize("case", cg.ANISOTROPIC, ids=IDS)
def test_anisotropic_case_differs_from_every_swapped_variant(case):
    """Swapping the strides, the dilations, the leading pads or the kernel (its weights transposed with it) between the
    axes changes the output's shape or moves it by more than 0.1 in relative L2: an H/W swap is an error of order 1."""
    b, h, w, ci, co, k, s, pad, d = cg.norm(case.geom)
    host, ref = cg.reference(case.geom)
    variants = cg.swapped_variants(case.geom)
    assert variants, "nothing differs between the axes"
    assert k[0] != k[1] or s[0] != s[1] or d[0] != d[1] or isinstance(pad, tuple)
    x = torch.relu(host["x"] * host["sc"] + host["sh"]).double()
    for what, geom, transposed in variants:
        wt = host["w"].double()
        if transposed:
            wt = wt.transpose(0, 1).contiguous()
        try:
            y = cg.oracle_conv(x, wt, None, geom)
        except RuntimeError:      # the swapped geometry has no output at all
            continue
        if tuple(y.shape) != tuple(ref["y_pro"].shape):
            continue
        assert cg.rel_l2(y, ref["y_pro"]) > 0.1, (what, cg.rel_l2(y, ref["y_pro"]))


def test_anisotropic_list_holds_what_it_is_there_for():
    geoms = [cg.norm(c.geom) for c in cg.ANISOTROPIC]
    pads = [cg.explicit_pads(c.geom) for c in cg.ANISOTROPIC]
    assert ((0, 0), (1, 1)) in pads and ((1, 1), (0, 0)) in pads                    # pad_top 0 / pad_left 1 and the reverse
    assert any(p[0][0] == 1 and p[1][0] == 3 for p in pads) and any(p[0][0] == 2 and p[1][0] == 0 for p in pads)
    assert ((2, 0), (0, 1)) in pads
    for want in ((2, 1), (1, 2)):
        assert any(g[6] == want and g[5] == (3, 3) for g in geoms) and any(g[6] == want and g[5] == (1, 1) for g in geoms)
    assert any(g[8] == (1, 3) for g in geoms) and any(g[8] == (2, 1) for g in geoms)
    assert all(g[1] != g[2] for g in geoms)                                             # no square map
    # the 1x1 cases with unequal strides are not the scatter form, and their weight gradient is not bounds-free
    for c in cg.ANISOTROPIC:
        if cg.norm(c.geom)[5] == (1, 1):
            assert not cg.dgrad_is_strided_1x1(c.geom)
            l = cg.launch("wgrad", c.geom)
            assert [cg.gather_variant(2, bm, l.gather) for bm in (128, 64)] == [0, 3]
            assert cg.gather_variant(0, 128, cg.launch("fwd", c.geom).gather) == 1
    # unequal strides under the pixel walk: an output row does not divide a K-step, so the row carry (dj_walk.h, c1) is taken
    walked = [c for c in cg.ANISOTROPIC if cg.norm(c.geom)[6][0] != cg.norm(c.geom)[6][1] and 3 in c.np[2:]]
    assert {cg.norm(c.geom)[6] for c in walked} == {(2, 1), (1, 2)}
    for c in walked:
        ow = cg.out_size(c.geom)[1]
        assert 16 % ow and 32 % ow, c.geom
    for t in cg.TRANSPOSE:
        b, h, w, ci, co, k, s = t
        geom = cg.transpose_conv_geom(t)
        assert cg.out_size(geom) == (h, w) and k[0] != k[1] or s[0] != s[1]
        y = ko.conv2d_transpose(torch.zeros(b, h, w, ci), torch.zeros(k[0], k[1], co, ci), None, s)
        assert tuple(y.shape) == (b, geom[1], geom[2], co)
        assert not cg.dgrad_is_strided_1x1(geom)
    assert [t[5:] for t in cg.TRANSPOSE] == [((2, 3), (2, 3)), ((3, 3), (2, 1))]


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_routing_predicate_gives_what_the_case_names(case):
    for role in cg.ROLES:
        assert cg.route(role, case.geom, case.layout) == case.route[role], role
        l = cg.launch(role, case.geom, case.layout, prologue=True)
        assert l.fast == (2 if case.route[role] == "fast" else 0)
        assert cg.launch(role, case.geom, case.layout, allow_fast=False).fast == 0
    assert cg.gather_variants_of(case) == case.np
    # a bias turns the scatter form into the plain input gradient (Conv2DTranspose with a bias)
    if case.route["dgrad"].startswith("scatter"):
        assert not cg.launch("dgrad", case.geom, case.layout, bias=True).scatter
    # dj_set_gather_variants(0): the tap cache and the walk go, the bounds-free 1x1 variant stays
    for role, bm in (("fwd", 128), ("wgrad", 64)):
        l = cg.launch(role, case.geom, case.layout)
        assert cg.gather_variant(l.am, bm, l.gather, variants=False) in (0, 1)


def test_one_clause_of_fast_mode_at_a_time():
    """The minimally ineligible geometries of the routing test and their eligible twins."""
    base = (2, 6, 7, 64, 64, 3, 1, "same", 1)
    assert all(cg.route(r, base) == "fast" for r in cg.ROLES)
    assert cg.route("fwd", (2, 6, 7, 48, 64, 3, 1, "same", 1)) == "generic:vv"          # Cin % 32
    assert cg.route("wgrad", (2, 6, 7, 48, 64, 3, 1, "same", 1)) == "fast"              # (the weight gradient: Cin % 4)
    assert cg.route("wgrad", (2, 6, 7, 62, 64, 3, 1, "same", 1)) == "generic:sv"
    assert cg.route("fwd", (2, 6, 7, 64, 62, 3, 1, "same", 1)) == "generic:vs"          # N % 4
    assert cg.route("dgrad", (2, 6, 7, 64, 64, 3, 2, "same", 1)) == "generic:vv"        # input-gradient stride
    assert cg.route("dgrad", (2, 6, 7, 64, 48, 3, 1, "same", 1)) == "generic:vv"        # Cout % 32 of the input gradient
    assert cg.route("fwd", (2, 6, 7, 64, 48, 3, 1, "same", 1)) == "fast"
    assert cg.route("fwd", base, cg.Layout("ld", 65, 0, None, 0, 0)) == "generic:sv"    # ld % 4
    assert cg.route("fwd", base, cg.Layout("ld", 68, 0, None, 0, 0)) == "fast"
    assert cg.route("fwd", base, cg.Layout("off", 68, 4, None, 0, 0)) == "generic:sv"   # pointer alignment
    assert cg.route("fwd", base, cg.Layout("off", 68, 16, None, 0, 0)) == "fast"
    assert cg.route("wgrad", base, cg.Layout("ldy", None, 0, 66, 0, 0)) == "generic:vs"
    assert cg.route("dgrad", base, cg.Layout("offy", None, 0, 68, 8, 0)) == "generic:sv"


def test_generic_cases_reach_every_path():
    cov = cg.generic_coverage()
    missing = [c for c in cg.REQUIRED_COVERAGE if c not in cov]
    assert not missing, missing
    # and the square list by itself misses only the forward GEMM with both operands scalar
    square = cg.generic_coverage(cg.GENERIC)
    assert [c for c in cg.REQUIRED_COVERAGE if c not in square] == ["fwd:AsBs"]


def test_generic_cases_are_what_their_comments_say():
    by = {(c.geom[3], c.geom[4], c.layout.name): c for c in cg.GENERIC}
    l = cg.launch("wgrad", by[(3, 20, "dense")].geom)
    assert l.M == 27 and l.M < min(bm for bm, _ in cg.TILES)
    assert cg.launch("fwd", by[(24, 20, "dense")].geom).M == 126
    l = cg.launch("fwd", by[(24, 128, "dense")].geom)
    assert (l.M, l.N, l.K) == (646, 128, 216) and l.K // cg.DJ_BK == 6 and l.K % cg.DJ_BK == 24 and l.M // 128 == 5
    l = cg.launch("dgrad", by[(128, 24, "dense")].geom)
    assert (l.M, l.N, l.K) == (646, 128, 216)
    l = cg.launch("fwd", by[(4, 32, "dense")].geom)
    assert cg.DJ_BK // l.srcC == 8 and l.K == 196
    assert by[(64, 126, "dense")].geom[4] % 4 == 2
    for key in ((64, 24, "dense"), (64, 21, "dense")):
        l = cg.launch("dgrad", by[key].geom)
        assert l.scatter and (l.am, l.bmd) == (0, 1) and l.K == by[key].geom[4]
    assert cg.GENERIC_TILE_OF_CFG[9] == 0 and cg.GENERIC_TILE_OF_CFG[(cg.N_CFG + 2) - cg.N_CFG] == 2
    assert len(cg.GENERIC_KERNEL_CASES) == len(cg.GENERIC) + 2
