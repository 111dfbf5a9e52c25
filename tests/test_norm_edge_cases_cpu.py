"""What tests/test_norm_edges_gpu.py relies on, checked without a GPU: every case of tests/norm_edge_cases.py satisfies the
dispatch predicate of the path it names and the table reaches every path; dyadic data is exact in fp32 and has its zeros; the
numpy pooling reference agrees with the oracle; the L2Normalization rows sit where they are said to sit."""
import numpy as np
import pytest
import torch

import norm_edge_cases as nc
from oracle import keras_ops as ko


def test_every_required_path_has_a_case():
    reached = nc.path_witnesses()
    missing = [p for p in nc.REQUIRED_PATHS if not reached.get(p)]
    assert not missing, missing


@pytest.mark.parametrize("layout", nc.LAYOUTS, ids=lambda l: l.name)
@pytest.mark.parametrize("n_tensors", [1, 2, 3, 5])
def test_layout_reaches_the_path_it_names(layout, n_tensors):
    slabs = nc.layout_slabs(layout, n_tensors)
    assert nc.v4(layout.C, slabs, (layout.vec_off,)) == (layout.path == "v4")
    assert len({s.ld for s in slabs}) == n_tensors                      # a stride of its own for every tensor
    # one reason at a time: with that reason taken away the layout is on the 4-wide path
    if layout.name == "scalar_c":
        assert all(s.ld % 4 == 0 and nc.aligned16(s.off) for s in slabs) and layout.C % 4
    elif layout.name == "scalar_ld":
        assert layout.C % 4 == 0 and all(s.ld % 4 and s.off == 0 for s in slabs)
    elif layout.name.startswith("scalar_off"):
        assert layout.C % 4 == 0 and all(s.ld % 4 == 0 for s in slabs)
        assert [s.off % 4 != 0 for s in slabs].count(True) == 1
    elif layout.name == "scalar_vec":
        assert nc.v4(layout.C, slabs, (0,)) and not nc.aligned16(layout.vec_off)


def test_named_slice_layouts_are_the_ones_asked_for():
    L = nc.LAYOUT_BY_NAME
    assert (L["scalar_ld"].C, L["scalar_ld"].ld) == (8, 9)
    assert [(L["scalar_off%d" % k].C, L["scalar_off%d" % k].ld, L["scalar_off%d" % k].off) for k in (1, 2, 3)] == \
        [(8, 12, 1), (8, 12, 2), (8, 12, 3)]
    assert (L["v4_slice"].ld, L["v4_slice"].off) == (L["v4_slice"].C + 8, 4)


def test_colreduce_thread_shapes():
    assert [nc.tx_log2(C, True) for C in nc.COLRED_C_V4] == [2, 2, 3, 4, 5, 6]
    assert [nc.column_blocks(C, True) for C in nc.COLRED_C_V4] == [1, 1, 1, 1, 1, 2]
    assert 260 // 4 - 64 == 1                                            # the second column block has one live group
    assert [nc.tx_log2(C, False) for C in nc.COLRED_C_SCALAR] == [2, 2, 3, 5, 6]
    assert nc.column_blocks(65, False) == 2
    assert all(C % 4 == 0 for C in nc.COLRED_C_V4) and all(C % 4 for C in nc.COLRED_C_SCALAR)
    # rows: one short block, one row short of a block, a full block, a block and a row, many blocks with a short last one
    assert [-(-r // nc.RB) for r in nc.COLRED_ROWS] == [1, 1, 1, 2, 17] and 1083 % nc.RB


def test_finalizer_rows_straddle_the_unrolled_loop():
    assert nc.fin_lane_work(192, 0) == (0, 3) and nc.fin_lane_work(193, 0) == (1, 0) and nc.fin_lane_work(193, 1) == (0, 3)
    assert nc.fin_lane_work(256, 63) == (1, 0) and nc.fin_lane_work(257, 0) == (1, 1)
    assert nc.fin_lane_work(449, 0) == (2, 0) and nc.fin_lane_work(704, 0) == (2, 3)
    for n in nc.FIN_NROWS:      # every partial row is read by exactly one lane, once
        assert sum(4 * t + l for t, l in (nc.fin_lane_work(n, k) for k in range(nc.FIN_LANES))) == n
    # C around the 16 channels of a finalizer block
    assert [-(-C // nc.FIN_CH) for C in nc.FIN_C] == [1, 1, 1, 2, 3]


def test_finalizer_partials_hold_the_constant_and_the_clamped_column():
    for nrows in nc.FIN_NROWS:
        p = nc.fin_partials(nc.rng_for("fin", nrows), nrows, 17).astype(np.float64)
        count = 64.0 * nrows
        m, q = p[:, 0].sum(0) / count, p[:, 1].sum(0) / count
        var = q - m * m
        assert var[0] == 0.0 and var[1] < 0.0 and (var[2:] > 0.25).all()
        var32 = (np.float32(q[1]) - np.float32(m[1]) * np.float32(m[1]))
        assert var32 < 0


@pytest.mark.parametrize("rows,C", [(65, 8), (130, 30), (1, 1), (1083, 7)])
def test_dyadic_data_is_exact_and_has_its_zeros(rows, C):
    d = nc.dyadic_bn(nc.rng_for("dy", rows, C), rows, C)
    for k in ("z", "y", "dy", "shift", "mean", "k2"):
        assert np.array_equal(d[k] * 8, np.round(d[k] * 8)) and np.abs(d[k]).max() <= 8, k
    for k in ("scale", "invstd", "k0", "k1"):
        assert (np.frexp(d[k])[0].__abs__() == 0.5).all(), k            # powers of two
    pre32 = d["z"] * d["scale"] + d["shift"]                             # fp32 arithmetic
    pre64 = d["z"].astype(np.float64) * d["scale"].astype(np.float64) + d["shift"].astype(np.float64)
    assert pre32.dtype == np.float32 and np.array_equal(pre32.astype(np.float64), pre64)
    assert (pre64 == 0).any()
    if rows * C > 8:
        assert (pre64 > 0).any() and (pre64 < 0).any()
        assert (d["y"] == 0).any() and (d["y"] > 0).any() and (d["y"] < 0).any()
    # the backward terms and their block sums are exact in fp32 as well
    for mode in (0, 1, 2):
        g, gx = nc.ref_bn_bwd_terms(d, mode)
        part, _ = nc.ref_partials(g, gx)
        assert np.array_equal(part.astype(np.float32).astype(np.float64), part)
        assert np.array_equal(gx.astype(np.float32).astype(np.float64), gx)
        dz, _, _ = nc.ref_bn_bwd_apply(d, mode)
        assert np.array_equal(dz.astype(np.float32).astype(np.float64), dz)
    a = nc.affine_data("dyadic", nc.rng_for("af", rows, C), rows, C)
    v, _ = nc.ref_affine_act(a["x"], a["scale"], a["shift"], a["res"], a["rscale"], a["rshift"], 0)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    v32 = (a["x"] * a["scale"] + a["shift"]) + (a["res"] * a["rscale"] + a["rshift"])
    assert np.array_equal(v32.astype(np.float64), v)


def test_slab_views_and_surroundings():
    s = nc.Slab(5, 3, 7, 2)
    vals = np.arange(15, dtype=np.float32).reshape(5, 3)
    buf = s.host(vals)
    assert buf.size == s.size and np.array_equal(s.read(buf), vals)
    assert (buf.view(np.uint32)[:2] == nc.SENTINEL_BITS).all() and buf.view(np.uint32)[5] == nc.SENTINEL_BITS
    after = buf.copy()
    after[s.index] += 1
    assert s.surroundings_equal(buf, after)
    after[1] = 0.0
    assert not s.surroundings_equal(buf, after)
    after = buf.copy()
    after[s.off + s.ld * s.rows] = 1.0                                   # the first float after the last row
    assert not s.surroundings_equal(buf, after)


@pytest.mark.parametrize("data", nc.POOL_DATA)
@pytest.mark.parametrize("geom", nc.POOL_GEOMS, ids=lambda g: g.name)
def test_pool_reference_against_the_oracle(geom, data):
    x, dy, _ = nc.pool_input(geom, 6, data)
    assert geom.H != geom.W and geom.OH != geom.OW or geom.name == "2x2s3gaps"
    assert (geom.OH - 1) * geom.sh - geom.pt < geom.H and (geom.OW - 1) * geom.sw - geom.pl < geom.W
    for pad_zero in (0, 1):
        y, code = nc.ref_maxpool(x, geom, pad_zero)
        pb = max((geom.OH - 1) * geom.sh + geom.kh - geom.pt - geom.H, 0)
        pr = max((geom.OW - 1) * geom.sw + geom.kw - geom.pl - geom.W, 0)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        if pad_zero:    # a ZeroPadding2D in front of a 'valid' pooling
            yo = ko.max_pool(ko.zero_padding(xt, ((geom.pt, pb), (geom.pl, pr))), (geom.kh, geom.kw), (geom.sh, geom.sw))
        else:           # padding that never wins
            xp = torch.nn.functional.pad(xt.permute(0, 3, 1, 2), (geom.pl, pr, geom.pt, pb), value=float("-inf"))
            yo = ko.max_pool(xp.permute(0, 2, 3, 1), (geom.kh, geom.kw), (geom.sh, geom.sw))
        assert tuple(yo.shape) == y.shape
        assert np.array_equal(yo.detach().numpy(), y)
        yo.backward(torch.from_numpy(dy).double())
        # torch's CPU max_pool2d also routes the gradient to the first maximum in window order
        assert np.array_equal(xt.grad.numpy(), nc.ref_maxpool_bwd(code, dy, geom, x.shape))
        if data == "negative" and pad_zero and (geom.pt or pb):
            assert (code == 255).any()
        if data == "negative" and not pad_zero:
            assert not (code == 255).any()
    if geom.name == "3x3s2same6x7":
        assert ko.same_padding(geom.H, 3, 2)[0] == geom.pt and ko.same_padding(geom.W, 3, 2)[0] == geom.pl
        assert tuple(ko.max_pool(torch.from_numpy(x), (3, 3), (2, 2), "same").shape[1:3]) == (geom.OH, geom.OW)
        assert np.array_equal(ko.max_pool(torch.from_numpy(x), (3, 3), (2, 2), "same").numpy(), nc.ref_maxpool(x, geom, 0)[0])


def test_pool_ties_and_gaps():
    gaps = [g for g in nc.POOL_GEOMS if g.name == "2x2s3gaps"][0]
    unc = nc.pool_uncovered(gaps)
    assert unc[2].all() and unc[:, 2].all() and unc[:, 5].all() and unc[:, 6].all() and not unc[0, 0]
    assert not any(nc.pool_uncovered(g).any() for g in nc.POOL_GEOMS if g.name.startswith("3x3"))
    valid = nc.pool_uncovered([g for g in nc.POOL_GEOMS if g.name == "2x2s2valid"][0])     # the last row and column only
    assert valid[4].all() and valid[:, 6].all() and not valid[:4, :6].any()
    # ReLU-ed input with zero pads: somewhere a zero pad tap comes first in the window and ties with an in-image zero
    g = nc.POOL_GEOMS[0]
    x, _, _ = nc.pool_input(g, 4, "relu")
    y, code = nc.ref_maxpool(x, g, 1)
    assert ((y == 0) & (code == 255)).any() and ((y == 0) & (code != 255)).any()
    y0, code0 = nc.ref_maxpool(x, g, 0)
    assert not (code0 == 255).any() and np.array_equal(y, y0)


def test_anisotropic_pool_cases_hold_what_the_library_computes():
    """The two cases whose window and strides differ between the axes: pads and output size as conv_geometry resolves
    them, every pixel covered, and an H/W swap of the window or of the strides changes the output size or the pads."""
    from jpeg_detection_resnet_ssd_amd.kernels import conv_geometry
    by_name = {g.name: g for g in nc.POOL_GEOMS}
    assert set(nc.POOL_ANISOTROPIC) <= set(by_name)
    for name, padding in (("2x3s1x2", "valid"), ("3x2s2x1same", "same")):
        g = by_name[name]
        assert g.kh != g.kw and g.sh != g.sw
        assert conv_geometry(g.H, g.W, (g.kh, g.kw), (g.sh, g.sw), padding, (1, 1)) == (g.pt, g.pl, g.OH, g.OW)
        for kernel, strides in (((g.kw, g.kh), (g.sh, g.sw)), ((g.kh, g.kw), (g.sw, g.sh))):
            swapped = conv_geometry(g.H, g.W, kernel, strides, padding, (1, 1))
            assert swapped != (g.pt, g.pl, g.OH, g.OW)                     # ('same' keeps the size: the pads move)
            assert swapped[2:] != (g.OH, g.OW) or (padding == "same" and strides == (g.sh, g.sw))
    assert not nc.pool_uncovered(by_name["3x2s2x1same"]).any()
    unc = nc.pool_uncovered(by_name["2x3s1x2"])      # rows: windows at 0..3 of height 2 reach row 4; columns 0..6 all
    assert not unc.any()


def test_pool_paths():
    assert nc.pool4(4, 4, 4, None) and nc.pool4(4, 4, 4, 0) and not nc.pool4(4, 4, 4, 1) and not nc.pool4(6, 4, 4, 0)
    assert [nc.pool_bwd_path(4, 4, 4, a) for a in nc.POOL_ARGMAX] == ["bwd_rescan", "bwd4", "bwd_saved_scalar"]
    assert nc.pool_bwd_path(6, 4, 4, 0) == "bwd_saved_scalar"


@pytest.mark.parametrize("C", nc.L2_C)
def test_l2_rows_sit_where_they_are_said_to(C):
    x, gamma, dy, _ = nc.l2_input(C)
    ss32, ss64 = nc.l2_sumsq(x, np.float32), nc.l2_sumsq(x, np.float64)
    assert ss32.dtype == np.float32
    for ss in (ss32.astype(np.float64), ss64):
        assert ss[nc.L2_ZERO_ROW] == 0
        assert all(0 < ss[r] < 1e-13 for r in nc.L2_CLAMP_ROWS)
        assert all(1e-10 <= ss[r] <= 1e-8 for r in nc.L2_ABOVE_ROWS)
        rest = [r for r in range(nc.L2_ROWS) if r not in (nc.L2_ZERO_ROW,) + nc.L2_CLAMP_ROWS + nc.L2_ABOVE_ROWS]
        assert all(ss[r] > 1 for r in rest)
    # in the clamped rows the two branches of the backward differ by far more than the tolerance
    for r in nc.L2_CLAMP_ROWS:
        xh = x[r].astype(np.float64) * 1e6
        g = dy[r].astype(np.float64) * gamma
        diff = 1e6 * np.abs(xh * (g * xh).sum())
        assert diff.max() > 20 * nc.l2_rel(C, 3) * 1e6 * np.abs(g).max()


def test_multi_part_tables():
    parts = nc.COPY_PARTS_TABLE
    assert len(parts) == nc.COPY_PARTS + 1 and nc.COPY_PART_COUNTS == [1, nc.COPY_PARTS, nc.COPY_PARTS + 1]
    sizes = [p[0] * p[1] for p in parts]
    assert not nc.copy_part_v4(parts[int(np.argmax(sizes))]) and min(sizes) == 1
    assert {nc.copy_part_v4(p) for p in parts[:8]} == {True, False}
    assert nc.COLSUM_PART_COUNTS == [1, nc.COLSUM_PARTS, nc.COLSUM_PARTS + 1]
    cs = [c for _, c, _ in nc.colsum_parts(32)]
    assert -(-max(cs) // nc.FIN_CH) > -(-min(cs) // nc.FIN_CH)            # blocks past a small part's C return early
