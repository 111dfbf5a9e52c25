"""What tests/test_loss_head_gpu.py relies on, checked without a GPU: the table of tests/loss_head_cases.py reaches every path
it lists and each case satisfies the predicate of the path it names; the numpy references agree with the oracle; dyadic data
is exact in fp32; the mining cases hold the clusters, tie groups and zero losses they are said to hold (losses computed here
in fp32); no input sits at a clip or branch boundary, so that no element has to be left out of a comparison."""
import numpy as np
import pytest
import torch

import loss_head_cases as lc
from oracle import keras_ops as ko


def test_every_required_path_has_a_case():
    reached = lc.path_witnesses()
    missing = [p for p in lc.REQUIRED_PATHS if not reached.get(p)]
    assert not missing, missing
    assert len(set(lc.REQUIRED_PATHS)) == len(lc.REQUIRED_PATHS)


def test_softmax_shapes_reach_the_paths_they_name():
    assert [lc.softmax_group(C) for C in lc.SOFTMAX_C] == [8, 8, 8, 16, 16, 32, 32, 32, 64, 64, 64, 64]
    assert [lc.softmax_rows_per_block(C) for C in (8, 16, 32, 64)] == [32, 16, 8, 4]
    assert sorted(lc.softmax_group(C) for C in lc.SOFTMAX_BIG_C) == [8, 16, 32, 64]
    for C in lc.SOFTMAX_C:
        G, rpb = lc.softmax_group(C), lc.softmax_rows_per_block(C)
        rows = lc.softmax_rows(C)
        assert rows == [1, rpb - 1, rpb + 1, 3 * rpb + 2] and all(r % rpb for r in rows)      # every one has a dead tail
        assert [-(-r // rpb) for r in rows] == [1, 1, 2, 4]
        if G < 64:      # a wave that holds live and dead sub-rows: in three of the four at least (26 rows of G = 32 fill it)
            assert sum(1 for r in rows if r % (64 // G)) >= 3
    assert 65 % 64 == 1 and 130 % 64 == 2
    x, _, _ = lc.softmax_input(5, 21, big=True)
    assert (x.max(1) == 90).all() and (np.abs(np.abs(x) - 80) <= 1).sum() == 5 * 20
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(x.max(1))).all()            # without the max subtraction the row overflows
    p = lc.ref_softmax(x)
    assert np.isfinite(p).all() and (p.max(1) > 0.9).all() and ((p > 1e-6) & (p < 0.1)).any()


@pytest.mark.parametrize("rows,C", [(5, 7), (3, 65)])
def test_softmax_backward_reference_is_autograd_of_the_oracle(rows, C):
    x, dp, dx0 = lc.softmax_input(rows, C)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    pt = ko.softmax(xt)
    pt.backward(torch.from_numpy(dp).double())
    ref = lc.ref_softmax_bwd(pt.detach().numpy(), dp, dx0, 0)
    np.testing.assert_allclose(ref, xt.grad.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(lc.ref_softmax_bwd(pt.detach().numpy(), dp, dx0, 1), ref + dx0.astype(np.float64))


def test_bound_rule():
    ref = np.array([1.0, 2.0, 0.0])
    assert lc.rel_err(ref, ref, np.abs(ref)) == 0
    assert lc.rel_err([1.0, 2.0, 1e-30], ref, np.abs(ref)) == np.inf         # a zero of the reference must be matched
    assert lc.rel_err([1.0, 2.5, 0.0], ref, np.abs(ref)) == 0.25
    assert not lc.rel_err([1.0, np.nan, 0.0], ref, np.abs(ref)) <= 1e30       # a NaN never passes
    assert lc.bound(ref, ref, np.abs(ref)) == lc.FLOOR == 2.0 ** -21
    assert lc.bound([1.0, 2.0 + 2e-6, 0.0], ref, np.abs(ref)) == pytest.approx(8e-6)


def test_gap_cases():
    big = lc.GAP_SHAPES[-1]
    assert big[0] * big[2] > 4096 * 256 and lc.ew_blocks(big[0] * big[2]) == 4096 and lc.GAP_SHAPES[0] == (1, 1, 1)
    for B, HW, C in lc.GAP_SHAPES[:3]:
        for kind in lc.gap_kinds(HW):
            x, dy, dx0 = lc.gap_input(B, HW, C, kind)
            xt = torch.from_numpy(x).double().reshape(B, HW, 1, C).requires_grad_(True)
            yt = ko.global_average_pooling(xt)
            yt.backward(torch.from_numpy(dy).double())
            np.testing.assert_array_equal(lc.ref_gap_fwd(x), yt.detach().numpy())
            np.testing.assert_allclose(lc.ref_gap_bwd(dy, HW, dx0, 0), xt.grad.numpy().reshape(B, HW, C), rtol=1e-15)
            if kind == "dyadic":     # exact in fp32, forward and backward, with and without the old dx
                assert HW & (HW - 1) == 0
                for ref in (lc.ref_gap_fwd(x), lc.ref_gap_bwd(dy, HW, dx0, 0), lc.ref_gap_bwd(dy, HW, dx0, 1)):
                    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
                assert np.array_equal(lc.ref_gap_fwd(x, torch.float32).astype(np.float64), lc.ref_gap_fwd(x))
    assert lc.gap_kinds(49) == ["normal"] and lc.gap_kinds(64) == ["dyadic", "normal"]


def test_sgd_cases():
    assert lc.SGD_GROUPS_PER_PASS == 2048 * 256 and lc.SGD_N == [1, 63, 257, 4 * 2048 * 256 + 4003]
    assert [lc.sgd_groups(n) for n in (1, 4, 5)] == [1, 1, 2]
    assert lc.sgd_groups(lc.SGD_N[-1]) > lc.SGD_GROUPS_PER_PASS >= lc.sgd_groups(lc.SGD_N[-2])      # threads take a second group
    assert lc.SGD_N[-1] % 4 == 3                                                                    # and the last group is partial
    for kind in lc.SGD_SCALARS:
        full = lc.sgd_configs(257, kind)
        assert len(set(full)) == 32
        few = lc.sgd_configs(lc.SGD_N[-1], kind)
        for nes in (0, 1):
            for field in ("momentum", "l2", "grad_scale", "sumsq"):
                assert len({getattr(c, field) for c in few if c.nesterov == nes}) == 2, field
    lr_t, moms, l2s, gss = lc.SGD_SCALARS["dyadic"]
    assert all(v == 0 or np.frexp(v)[0] == 0.5 for v in (lr_t,) + moms + l2s + gss)            # powers of two
    assert lc.SGD_SCALARS["normal"][1:] == ((0.0, 0.9), (0.0, 5e-4), (1.0, 0.125))
    p, g, v = lc.sgd_input(257, "dyadic")
    for cfg in lc.sgd_configs(257, "dyadic"):       # exact in fp32: the fp32 evaluation equals the float64 one
        p64, v64 = lc.ref_sgd(p, g, v, cfg)
        p32, v32 = lc.ref_sgd(p, g, v, cfg, torch.float32)
        assert np.array_equal(p32.astype(np.float64), p64) and np.array_equal(v32.astype(np.float64), v64)
    # the reference is the oracle's step on the effective gradient
    p, g, v = lc.sgd_input(63, "normal")
    cfg = lc.SgdCfg(0.1, 0.9, 1, 5e-4, 0.125, True)
    f = lc.f32val
    g_eff = torch.from_numpy(g).double() * f(0.125) + 2 * f(5e-4) * torch.from_numpy(p).double()
    pn, vn = ko.sgd_keras_step(torch.from_numpy(p).double(), g_eff, torch.from_numpy(v).double(), f(0.1), f(0.9), 0.0, 0, True)
    p64, v64 = lc.ref_sgd(p, g, v, cfg)
    assert np.array_equal(p64, pn.numpy()) and np.array_equal(v64, vn.numpy())
    sp, sv = lc.sgd_scales(p, g, v, cfg)
    assert (sp >= np.abs(p64)).all() and (sv >= np.abs(v64)).all()
    assert lc.ref_sumsq(p) == lc.SGD_SUMSQ0 + (p.astype(np.float64) ** 2).sum() and lc.SGD_SUMSQ0 != 0


@pytest.mark.parametrize("rows,C", lc.CCE_SHAPES)
def test_cce_cases_sit_away_from_the_clip(rows, C):
    for labels, scaled in [(l, s) for l in lc.CCE_LABELS for s in (False, True)]:
        y, p, lab = lc.cce_input(rows, C, labels, scaled)
        q = lc.cce_q(p)
        q32 = p / p.sum(axis=1, keepdims=True, dtype=np.float32)
        special = np.zeros((rows, C), dtype=bool)
        if labels == "onehot" and rows >= 3:
            special[lc.CCE_TINY_ROW, lab[lc.CCE_TINY_ROW]] = special[lc.CCE_ONE_ROW] = True
            assert abs(q[lc.CCE_TINY_ROW, lab[lc.CCE_TINY_ROW]] / 1e-9 - 1) < 1e-6
            assert q[lc.CCE_ONE_ROW, lab[lc.CCE_ONE_ROW]] == 1 and q32[lc.CCE_ONE_ROW, lab[lc.CCE_ONE_ROW]] == 1
        for qq in (q, q32.astype(np.float64)):      # nothing within a factor of ten of 1e-7, nothing within 1e-6 of 1
            rest = qq[~special]
            assert ((rest > 1e-6) & (rest < 1 - 1e-6)).all() or C == 1
            assert not ((qq > 1e-8) & (qq < 1e-6)).any() and not ((qq > 1 - 1e-6) & (qq < 1)).any()
        s = p.astype(np.float64).sum(1)
        if scaled:
            assert (s >= 0.24).all() and (s <= 4.1).all() and (np.abs(s - 1) > 1e-3).all()
        else:
            assert (np.abs(s - 1) < 1e-5)[~special.any(1)].all()
        if labels == "soft":
            assert np.allclose(y.sum(1), 1.0 if C > 1 else 0.9) and (y > 0).all()
        loss, mean, grad = lc.ref_cce(y, p, -2.0)
        assert np.isfinite(loss).all() and np.isfinite(grad).all()
        if labels == "onehot" and rows >= 3:
            assert loss[lc.CCE_TINY_ROW] == -np.log(1e-7) and loss[lc.CCE_ONE_ROW] == -np.log(1 - 1e-7)
            assert (grad[lc.CCE_TINY_ROW] == 0).all() and (grad[lc.CCE_ONE_ROW] == 0).all()
            assert (np.abs(grad[2:]).max(1) > 0).all()


def test_cce_gradient_reference_is_the_stated_formula():
    """Away from the clip, autograd of the oracle is (g/S - sum(g p)/S^2) * upstream / rows with g = -y / q."""
    y, p, _ = lc.cce_input(9, 1000, "soft", True)
    _, _, grad = lc.ref_cce(y, p, -2.0)
    p64, y64 = p.astype(np.float64), y.astype(np.float64)
    S = p64.sum(1, keepdims=True)
    g = -y64 / (p64 / S)
    want = (g / S - (g * p64).sum(1, keepdims=True) / (S * S)) * (-2.0 / 9)
    np.testing.assert_allclose(grad, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("n_cls", lc.SSD_NCLS)
@pytest.mark.parametrize("nbox", lc.SSD_NBOX)
def test_ssd_case_holds_what_it_names_and_matches_the_oracle(nbox, n_cls):
    c = lc.ssd_case(n_cls, nbox)
    assert c.y_true.shape == c.y_pred.shape == (nbox, n_cls + 12) and c.y_true.dtype == np.float32
    parts = lc.ssd_parts(c.y_true, c.y_pred)
    # the localisation differences are exact in fp32 and hold every special value
    d32 = c.y_true[:, n_cls:n_cls + 4] - c.y_pred[:, n_cls:n_cls + 4]
    assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), c.loc_diff)
    assert set(lc.LOC_SPECIAL[:4 * nbox]) <= set(c.loc_diff.reshape(-1).tolist())
    assert {0.0, 1.0, -1.0, 1 - 2.0 ** -20, -(1 - 2.0 ** -20), 1.5, -1.5} == set(lc.LOC_SPECIAL)
    if nbox > 1:
        assert (parts["pos"] == 1).sum() >= 2 and ((parts["pos"] == 0) & (parts["neg"] == 0)).any()
        assert ((parts["negloss"] == 0) & (parts["neg"] == 1)).any()          # negatives with p[0] == 1
        a, b = c.clamp_boxes
        assert parts["pos"][a] == parts["pos"][b] == 1
        tc = int(np.argmax(c.y_true[a, :n_cls])), int(np.argmax(c.y_true[b, :n_cls]))
        assert c.y_pred[a, tc[0]] == 0 and c.y_pred[b, tc[1]] == np.float32(1e-20)
        assert parts["cls"][a] == parts["cls"][b] == -np.log(1e-15)
        # no other probability of a labelled class is anywhere near the clamp
        lab = (c.y_true[:, :n_cls] != 0) & ~np.isin(np.arange(nbox), [a, b])[:, None]
        assert (c.y_pred[:, :n_cls][lab] > 1e-12).all()
    # the loss with the oracle's own keep set is the oracle's loss
    yt, yp = torch.from_numpy(c.y_true).double()[None], torch.from_numpy(c.y_pred).double()[None].requires_grad_(True)
    for ratio, nmin, alpha in [(3, 0, 1.0), (1, 40, 0.25)]:
        total, op = ko.ssd_loss(yt, yp, ratio, nmin, alpha, return_parts=True)
        for name, oname in [("cls", "cls"), ("loc", "loc"), ("pos", "positives"), ("neg", "negatives")]:
            assert np.array_equal(parts[name], op[oname].detach().numpy()[0]), name
        nnz = int((parts["negloss"] != 0).sum())
        assert lc.expected_k(parts["pos"].sum(), ratio, nmin, nnz) == op["n_keep"]
        keep = op["keep"].numpy()[0]
        assert lc.check_keep(parts["negloss"].astype(np.float32), keep, op["n_keep"]) == op["n_keep"] \
            or len(np.unique(parts["negloss"].astype(np.float32))) < len(np.unique(parts["negloss"]))
        out0, _, _ = lc.ssd_loss_with_keep(parts, keep, alpha)
        assert abs(out0 - float(total[0].detach())) <= 1e-13 * abs(out0)
        yp.grad = None
        (total[0] * -0.5).backward()
        np.testing.assert_allclose(lc.ssd_grad_with_keep(c.y_true, c.y_pred, keep, alpha, -0.5), yp.grad.numpy()[0],
                                   rtol=1e-12, atol=0)


def test_check_keep_rejects_wrong_sets():
    s = np.array([0.0, 3.0, 1.0, 1.0, 1.0, 2.0, 0.0], dtype=np.float32)
    good = np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.float32)
    assert lc.check_keep(s, good, 3) == 3
    assert lc.check_keep(s, [0, 1, 1, 1, 1, 1, 0], 9) == 5            # k above nnz: every non-zero loss, never a zero
    assert lc.check_keep(s, np.zeros(7), 0) == 0
    for bad, k in [([0, 1, 1, 1, 0, 1, 0], 3),       # one tie too many
                   ([0, 1, 0, 0, 0, 1, 0], 3),       # one too few
                   ([0, 0, 1, 1, 0, 1, 0], 3),       # the largest left out
                   ([1, 1, 0, 0, 0, 1, 0], 3),       # a zero loss kept
                   ([1, 1, 1, 1, 1, 1, 0], 9)]:
        with pytest.raises(AssertionError):
            lc.check_keep(s, bad, k)


def test_mining_case_structure():
    c = lc.mining_case()
    parts = lc.ssd_parts(c.y_true, c.y_pred)
    assert 550 <= c.nbox <= 650 and c.n_cls == lc.MINE_NCLS
    assert (parts["pos"] == 1).sum() == 8 and ((parts["pos"] == 0) & (parts["neg"] == 0)).sum() == 8
    s32 = lc.fp32_negloss(c)
    assert s32.dtype == np.float32
    m = lc.mining_structure(s32)
    assert m["zeros"] - 16 >= 10 and m["zeros"] - 16 == lc.MINE_ZERO_LOSS      # 16 boxes are no negatives at all
    assert m["binades"] >= 20
    assert m["top22"] >= 16 and m["top11"] >= 64
    assert {5, 64} <= set(m["ties"]) and m["ties"].count(2) >= 2 and m["ties"].count(64) == 1 and m["ties"].count(5) == 1
    # the cluster: at least 64 distinct values under one top-11 pattern, the tie group of 5 among them
    b = lc.bits_of(np.unique(s32[s32 != 0]))
    hi = lc.bits1(np.float32(0.7)) >> 21
    assert len(np.unique(b[(b >> 21) == hi])) >= 64 + 32
    five = np.float32(-np.log(np.float64(np.float32(lc.MINE_TIES[5]))))
    assert lc.bits1(five) >> 21 == hi
    # the run: 64 consecutive fp32 values of p[0], about half on either side of a multiple of 1024 ulp of the loss
    run_lo = lc.bits1(lc.p0_for_loss_bits(lc.MINE_RUN_START_BITS))
    pb = lc.bits_of(c.y_pred[:, 0])
    assert all((pb == run_lo - j).sum() == (2 if j == 20 else 1) for j in range(lc.MINE_RUN))
    run_loss = lc.bits_of(s32[(pb <= run_lo) & (pb > run_lo - lc.MINE_RUN) & (parts["neg"] == 1)])
    groups = np.unique(run_loss >> 10, return_counts=True)
    assert len(groups[0]) == 2 and (np.array([len(np.unique(run_loss[run_loss >> 10 == g])) for g in groups[0]]) >= 16).all()
    paths = lc.scan_paths(m["scan"])
    assert {"mine_scan_l1_thread0", "mine_scan_l1_thread255", "mine_scan_l2_thread0", "mine_scan_l2_thread255",
            "mine_scan_first_bin_of_run", "mine_scan_last_bin_of_run"} <= paths
    for bits, field in zip(lc.MINE_L1_EXTREME_BITS, (2044, 3)):
        assert (bits >> 10) & 2047 == field and bits >> 21 == hi
        got = lc.bits1(np.float32(-np.log(np.float64(lc.p0_for_loss_bits(bits)))))
        assert abs(got - bits) <= 2 and (s32.view(np.uint32) == got).sum() == 1


def test_mining_large_case_structure():
    c = lc.mining_large_case()
    assert c.nbox == 4 * 40000 and c.nbox > lc.LOSS_BLOCKS * lc.THREADS > lc.MINE_BLOCKS * lc.THREADS
    assert lc.loss_blocks(c.nbox) == 512 and lc.mine_blocks(c.nbox) == 256
    s32 = lc.fp32_negloss(c)
    sizes = lc.tie_class_sizes(s32)
    assert len(sizes) == 7 and sizes.min() > 20000
    parts = lc.ssd_parts(c.y_true, c.y_pred)
    assert np.array_equal(lc.tie_class_sizes(parts["negloss"]), sizes)
    assert parts["pos"].sum() == 40 and ((parts["negloss"] == 0) & (parts["neg"] == 1)).sum() > 1000
    # every tie class has members in every mine block: block b of 256 takes the boxes i with (i // 256) % 256 == b
    blk = (np.arange(c.nbox) // lc.THREADS) % lc.MINE_BLOCKS
    for v in np.unique(s32[s32 != 0]):
        assert len(np.unique(blk[s32 == v])) == lc.MINE_BLOCKS
    ks = lc.mining_large_ks(s32)
    b = int(sizes[0] + sizes[1])
    assert ks == [1, b - 1, b, b + 1, int(sizes.sum())] and len(c.clamp_boxes) == 2


def test_no_positive_and_ratio_cases():
    c = lc.no_positive_case()
    parts = lc.ssd_parts(c.y_true, c.y_pred)
    assert parts["pos"].sum() == 0 and (parts["negloss"] != 0).sum() > 100
    base = lc.ssd_parts(lc.ssd_case(21, 257).y_true, lc.ssd_case(21, 257).y_pred)
    assert np.array_equal(base["negloss"], parts["negloss"]) and base["pos"].sum() == 26
    nnz = int((base["negloss"] != 0).sum())
    ks = [lc.expected_k(26, r, m, nnz) for r, m in lc.MINE_RATIO_CASES]
    assert ks == [26, 26, 40, 78, 78, 100] and nnz > 100
    assert lc.expected_k(0, 3, 5, nnz) == 5 and lc.expected_k(0, 3, 0, nnz) == 0


def test_workspace_size_rule():
    assert lc.ssd_workspace_floats(1) == 5 + 2048 + 256 + 6144 + 16
    assert [lc.loss_blocks(n) for n in (1, 255, 257, 131072, 131073)] == [1, 1, 2, 512, 512]
    assert [lc.mine_blocks(n) for n in (1, 257, 65536, 65537)] == [1, 2, 256, 256]
    assert lc.scan_position(0x7FF << 21, 0) == (0, 0, 8) and lc.scan_position(0, 0) == (255, 7, 8)
    assert lc.scan_position(1023, 2) == (0, 0, 4) and lc.scan_position(4, 2) == (254, 3, 4)
