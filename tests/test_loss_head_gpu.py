"""Every code path of csrc/dj_loss.hip, and the SGD rule of csrc/dj_optim.hip, against the float64 references of tests/loss_head_cases.py: the dead tail and every
group size of the softmax kernels, the per-box pass, the mining selection at every k of a case built around its three radix
levels and its tie tickets, the backward of the SSD loss, categorical cross-entropy at its clips, the SGD update and global
average pooling past their grids.

Every output is a view into a NaN-filled buffer (`Dev`); after a launch everything around it must be unchanged bit for bit
and every input untouched.  Results that are exact by construction must EQUAL the reference; the others stay within the bound
that loss_head_cases.py derives from the fp32 evaluation of the reference (its docstring has the rule).  No element is left
out of a comparison.  Each check prints its error / bound when it is the largest of its kernel family so far."""
import numpy as np
import pytest
import torch

import loss_head_cases as lc
from loss_head_cases import Slab

pytestmark = pytest.mark.gpu
F32 = torch.float32
RATIOS = {}


@pytest.fixture()
def E(cuda):
    from jpeg_detection_resnet_ssd_amd import engine
    return engine


class Dev(object):
    """A slab on the device."""

    def __init__(self, slab, values, device):
        self.slab = slab
        self.before = slab.host(values)
        self.t = torch.from_numpy(self.before.copy()).to(device)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.slab.off

    @property
    def ld(self):
        return self.slab.ld

    def result(self):
        after = self.t.cpu().numpy()
        assert self.slab.surroundings_equal(self.before, after), "a write outside the output view"
        return self.slab.read(after)

    def untouched(self):
        return bool(np.array_equal(self.before.view(np.int32), self.t.cpu().numpy().view(np.int32)))


def dense(values, device, off=1, tail=None):
    values = np.asarray(values, dtype=np.float32)
    values = values.reshape(1, -1) if values.ndim < 2 else values.reshape(-1, values.shape[-1])
    return Dev(Slab(values.shape[0], values.shape[1], values.shape[1], off, tail), values, device)


def blank(rows, C, device, off=1, tail=None):
    return Dev(Slab(rows, C, C, off, tail), None, device)


def untouched(*devs):
    return all(d.untouched() for d in devs if d is not None)


def within(got, ref64, ref32, scale, family, what):
    b = lc.bound(ref32, ref64, scale)
    e = lc.rel_err(got, ref64, scale)
    if not e / b <= RATIOS.get(family, -1.0):
        RATIOS[family] = e / b
        print("error/bound %s (%s): %.3g / %.3g = %.3f" % (family, what, e, b, e / b))
    assert e <= b, "%s %s: error %.3g over the bound %.3g" % (family, what, e, b)


def assert_exact(got, ref64, what):
    ref64 = np.asarray(ref64, dtype=np.float64)
    want = ref64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref64), "reference not exact in fp32: " + what
    got = np.asarray(got).reshape(want.shape)
    assert np.array_equal(got, want), "%s: %d of %d elements differ" % (what, int((got != want).sum()), want.size)


def positive_zero(a):
    return not np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).any()


# ----------------------------------------------------------------------------------------------------------------------
# softmax
# ----------------------------------------------------------------------------------------------------------------------
def run_softmax(E, dev, rows, C, big):
    x0, dp0, dxold = lc.softmax_input(rows, C, big)
    guard = lc.softmax_rows_per_block(C) * C + 8        # the rows of a whole dead block, inside the allocation
    x, y = dense(x0, dev, 1, guard), blank(rows, C, dev, 3, guard)
    E.call("dj_softmax_fwd", x.ptr, y.ptr, rows, C)
    torch.cuda.synchronize()
    ref = lc.ref_softmax(x0)
    got = y.result()
    assert np.isfinite(got).all()
    within(got, ref, lc.ref_softmax(x0, F32), lc.row_max(ref), "softmax_fwd", "rows %d C %d big %d" % (rows, C, big))
    p0 = ref.astype(np.float32)
    p = dense(p0, dev, 2, guard)
    for extra in lc.SOFTMAX_LD_EXTRA:
        for beta in lc.SOFTMAX_BETA:
            dp = Dev(Slab(rows, C, C + extra, 1, 64 * rows + guard), dp0, dev)      # a column slice of a NaN-filled buffer
            dx = dense(dxold, dev, 1, guard) if beta else blank(rows, C, dev, 1, guard)
            E.call("dj_softmax_bwd", p.ptr, dp.ptr, dp.ld, dx.ptr, rows, C, beta)
            torch.cuda.synchronize()
            within(dx.result(), lc.ref_softmax_bwd(p0, dp0, dxold, beta), lc.ref_softmax_bwd(p0, dp0, dxold, beta, np.float32),
                   lc.softmax_bwd_scale(p0, dp0, dxold, beta), "softmax_bwd",
                   "rows %d C %d ld %d beta %d big %d" % (rows, C, C + extra, beta, big))
            assert dp.untouched()
    assert untouched(x, p)


@pytest.mark.parametrize("C", lc.SOFTMAX_C)
def test_softmax_tails_groups_strides_and_beta(C, cuda, E):
    for rows in lc.softmax_rows(C):
        run_softmax(E, cuda, rows, C, False)


@pytest.mark.parametrize("C", lc.SOFTMAX_BIG_C)
def test_softmax_logits_of_magnitude_80(C, cuda, E):
    run_softmax(E, cuda, lc.softmax_rows(C)[-1], C, True)


# ----------------------------------------------------------------------------------------------------------------------
# SSD loss
# ----------------------------------------------------------------------------------------------------------------------
class SsdRun(object):
    """The tensors of one case on the device, its float64 and fp32 per-box references, and the two entry points."""

    def __init__(self, E, dev, case):
        self.E, self.dev, self.case = E, dev, case
        self.n, self.n_cls = case.nbox, case.n_cls
        self.yt, self.yp = dense(case.y_true, dev), dense(case.y_pred, dev, 3)
        wsf = E.query("dj_ssd_loss_workspace_floats", self.n)
        assert wsf == lc.ssd_workspace_floats(self.n)
        self.ws = Dev(Slab(1, wsf, wsf, 0, 16), None, dev)
        self.out = Dev(Slab(1, 5, 5, 1, 8), None, dev)
        self.p64 = lc.ssd_parts(case.y_true, case.y_pred)
        self.p32 = lc.ssd_parts(case.y_true, case.y_pred, F32)
        self.n_pos = int(self.p64["pos"].sum())
        self.nnz = int((self.p64["negloss"] != 0).sum())

    def forward(self, ratio, nmin, alpha):
        self.E.call("dj_ssd_loss_fwd", self.yt.ptr, self.yp.ptr, self.n, self.n_cls, ratio, nmin, alpha, self.ws.ptr, self.out.ptr)
        torch.cuda.synchronize()
        ws, n = self.ws.result().reshape(-1), self.n        # .result(): the floats after the workspace and after out5 untouched
        res = dict(zip(("cls", "loc", "pos", "negloss", "keep"), (ws[j * n:(j + 1) * n] for j in range(5))))
        res["out"] = self.out.result().reshape(-1)
        return res

    def check_boxes(self, res):
        tag = "n_cls %d nbox %d" % (self.n_cls, self.n)
        for name in ("cls", "loc", "negloss"):
            within(res[name], self.p64[name], self.p32[name], np.abs(self.p64[name]), "ssd_boxes", name + " " + tag)
        assert_exact(res["pos"], self.p64["pos"], "pos")
        assert int((res["negloss"] != 0).sum()) == self.nnz
        for b in self.case.clamp_boxes:      # p = 0 and p = 1e-20 at the true class
            assert self.p64["cls"][b] == -np.log(1e-15)

    def check_forward(self, res, ratio, nmin, alpha):
        """out[1], out[2] and the keep set exactly; out[0], out[3], out[4] against the loss with that keep set."""
        out = res["out"]
        assert out[1] == self.n_pos
        assert out[2] == lc.expected_k(self.n_pos, ratio, nmin, self.nnz)
        assert lc.check_keep(res["negloss"], res["keep"], max(ratio * self.n_pos, nmin)) == out[2]
        assert not res["keep"][self.p64["neg"] == 0].any()
        r64 = lc.ssd_loss_with_keep(self.p64, res["keep"], lc.f32val(alpha))
        r32 = lc.ssd_loss_with_keep(self.p32, res["keep"], lc.f32val(alpha))
        for j, a, b in zip((0, 3, 4), r64, r32):
            within(out[j], a, b, abs(a), "ssd_loss", "out[%d] n_cls %d nbox %d k %d" % (j, self.n_cls, self.n, out[2]))
        return r64

    def check_backward(self, res, alpha, upstream):
        W = self.n_cls + 12
        d = blank(self.n, W, self.dev, 3)            # NaN-filled
        self.E.call("dj_ssd_loss_bwd", self.yt.ptr, self.yp.ptr, self.n, self.n_cls, alpha, upstream, self.ws.ptr,
                    self.out.ptr, d.ptr)
        torch.cuda.synchronize()
        got = d.result()
        c, keep = self.case, res["keep"]
        ref = lc.ssd_grad_with_keep(c.y_true, c.y_pred, keep, alpha, upstream)
        within(got, ref, lc.ssd_grad_with_keep(c.y_true, c.y_pred, keep, alpha, upstream, F32), np.abs(ref), "ssd_bwd",
               "n_cls %d nbox %d alpha %g upstream %g" % (self.n_cls, self.n, alpha, upstream))
        idle = (self.p64["pos"] == 0) & (keep == 0)
        assert positive_zero(got[idle]), "a row neither matched nor mined is not all +0"
        assert positive_zero(got[:, -8:]), "the anchor columns are not all +0"
        assert positive_zero(got[self.p64["pos"] == 0][:, self.n_cls:])
        for b in c.clamp_boxes:
            assert (got[b, :self.n_cls] == 0).all()
        return got

    def inputs_untouched(self):
        return untouched(self.yt, self.yp)


@pytest.mark.parametrize("nbox", lc.SSD_NBOX)
@pytest.mark.parametrize("n_cls", lc.SSD_NCLS)
def test_ssd_boxes_loss_and_backward(n_cls, nbox, cuda, E):
    run = SsdRun(E, cuda, lc.ssd_case(n_cls, nbox))
    for alpha in lc.SSD_ALPHA:
        res = run.forward(3, 0, alpha)
        run.check_boxes(res)
        run.check_forward(res, 3, 0, alpha)
        for upstream in lc.SSD_UPSTREAM:
            run.check_backward(res, alpha, upstream)
    assert run.inputs_untouched()


def test_mining_every_k(cuda, E):
    """k from 0 to nnz + 3 through n_neg_min (neg_pos_ratio 0) on the case built around the three radix levels."""
    run = SsdRun(E, cuda, lc.mining_case())
    res = run.forward(0, 0, 1.0)
    run.check_boxes(res)
    stored = res["negloss"].copy()
    m = lc.mining_structure(stored)       # what the device logf left of the structure
    assert m["top22"] >= 3 and m["top11"] >= 3 and {2, 5, 64} <= set(m["ties"]) and m["zeros"] >= 10 + 16
    assert {"mine_scan_l1_thread0", "mine_scan_l1_thread255", "mine_scan_l2_thread0", "mine_scan_l2_thread255",
            "mine_scan_first_bin_of_run", "mine_scan_last_bin_of_run"} <= lc.scan_paths(m["scan"])
    assert m["nnz"] == run.nnz
    for k in lc.mining_sweep(run.nnz):
        res = run.forward(0, k, 1.0)
        assert np.array_equal(res["negloss"], stored)
        run.check_forward(res, 0, k, 1.0)
    assert run.inputs_untouched()


_LARGE = {}


def large_run(E, dev):
    if "run" not in _LARGE:
        run = SsdRun(E, dev, lc.mining_large_case())
        res = run.forward(3, 0, 1.0)
        run.check_boxes(res)
        _LARGE["run"], _LARGE["ks"] = run, lc.mining_large_ks(res["negloss"])
        assert len(lc.tie_class_sizes(res["negloss"])) == lc.MINE_LARGE_CLASSES
    return _LARGE["run"], _LARGE["ks"]


@pytest.mark.parametrize("which", range(6))
def test_mining_ties_across_all_blocks(which, cuda, E):
    """160000 boxes whose negatives take seven loss values: the tickets of one tie class are drawn by all 256 blocks.
    k = 1, around a class boundary, nnz (through n_neg_min), and 3 * n_pos; with the backward."""
    run, ks = large_run(E, cuda)
    ratio, nmin = (0, ks[which]) if which < 5 else (3, 0)
    alpha, upstream = (1.0, 1.0) if which % 2 else (0.25, -0.5)
    res = run.forward(ratio, nmin, alpha)
    run.check_forward(res, ratio, nmin, alpha)
    run.check_backward(res, alpha, upstream)
    if which == 5:
        assert run.inputs_untouched()


def test_no_positives(cuda, E):
    run = SsdRun(E, cuda, lc.no_positive_case())
    assert run.n_pos == 0
    res = run.forward(3, 0, 1.0)
    run.check_forward(res, 3, 0, 1.0)
    assert positive_zero(res["out"]) and not res["keep"].any()
    got = run.check_backward(res, 1.0, 1.0)
    assert positive_zero(got)
    res = run.forward(3, 5, 0.25)
    r64 = run.check_forward(res, 3, 5, 0.25)
    assert res["out"][1] == 0 and res["out"][2] == 5 and res["keep"].sum() == 5
    assert abs(r64[0] - run.p64["cls"][res["keep"] != 0].sum()) <= 1e-12 * r64[0]        # a denominator of 1
    run.check_backward(res, 0.25, -0.5)


@pytest.mark.parametrize("ratio,nmin", lc.MINE_RATIO_CASES)
def test_ratio_and_n_neg_min(ratio, nmin, cuda, E):
    run = SsdRun(E, cuda, lc.ssd_case(21, 257))
    res = run.forward(ratio, nmin, 1.0)
    run.check_forward(res, ratio, nmin, 1.0)
    assert res["out"][2] == max(ratio * 26, nmin)
    run.check_backward(res, 1.0, 1.0)


# ----------------------------------------------------------------------------------------------------------------------
# categorical cross-entropy
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", lc.CCE_SHAPES)
def test_categorical_crossentropy(rows, C, cuda, E):
    for labels, scaled, given, upstream in lc.cce_variants():
        y0, p0, lab = lc.cce_input(rows, C, labels, scaled)
        tag = "rows %d C %d %s scaled %d d_probs %d upstream %g" % (rows, C, labels, scaled, given, upstream)
        y, p = dense(y0, cuda), dense(p0, cuda, 2)
        loss, mean = blank(1, rows, cuda), blank(1, 1, cuda)
        dp = blank(rows, C, cuda, 3) if given else None
        E.call("dj_categorical_crossentropy", y.ptr, p.ptr, rows, C, upstream, loss.ptr, dp.ptr if dp else None, mean.ptr)
        torch.cuda.synchronize()
        l64, m64, g64 = lc.ref_cce(y0, p0, upstream)
        l32, m32, g32 = lc.ref_cce(y0, p0, upstream, F32)
        within(loss.result(), l64, l32, np.abs(l64).max(), "cce", "loss_rows " + tag)
        within(mean.result(), m64, m32, abs(m64), "cce", "out_mean " + tag)
        if given:
            got = dp.result()
            within(got, g64, g32, lc.row_max(g64), "cce", "d_probs " + tag)
            if labels == "onehot" and rows >= 3:
                assert (got[[lc.CCE_TINY_ROW, lc.CCE_ONE_ROW]] == 0).all()
        assert untouched(y, p)


# ----------------------------------------------------------------------------------------------------------------------
# SGD
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(lc.SGD_SCALARS))
@pytest.mark.parametrize("n", lc.SGD_N)
def test_sgd(n, kind, cuda, E):
    """p, v and the sum of squares.  The three buffers sit at element offsets 1, 2 and 3 of their allocations, so every
    launch here takes the element-by-element path (tests/test_optimizers_gpu.py has the 16-byte one).  Past the grid (more
    groups of four than one pass of the capped grid covers) 2048 workgroups contribute to the sum: one fp32 atomic each on
    sumsq[0] would round the running total once per workgroup, different from run to run; the kernel adds the workgroups'
    sums in fp64 and rounds once."""
    assert lc.SGD_GROUPS_PER_PASS == E._lib.load().dj_optim_groups_per_pass()
    p0, g0, v0 = lc.sgd_input(n, kind)
    g = dense(g0, cuda, 3)
    for cfg in lc.sgd_configs(n, kind):
        tag = "n %d %s %s" % (n, kind, cfg)
        p, v = dense(p0, cuda), dense(v0, cuda, 2)
        ss = dense([lc.SGD_SUMSQ0], cuda) if cfg.sumsq else None
        E.call("dj_sgd_momentum_update", p.ptr, g.ptr, v.ptr, n, cfg.lr_t, cfg.momentum, cfg.nesterov, cfg.l2,
               cfg.grad_scale, ss.ptr if ss else None)
        torch.cuda.synchronize()
        p64, v64 = lc.ref_sgd(p0, g0, v0, cfg)
        if kind == "dyadic":
            assert_exact(p.result(), p64, "p " + tag)
            assert_exact(v.result(), v64, "v " + tag)
        else:
            p32, v32 = lc.ref_sgd(p0, g0, v0, cfg, F32)
            sp, sv = lc.sgd_scales(p0, g0, v0, cfg)
            within(p.result(), p64, p32, sp, "sgd", "p " + tag)
            within(v.result(), v64, v32, sv, "sgd", "v " + tag)
        if ss is not None:
            ref = lc.ref_sumsq(p0)
            within(ss.result(), ref, lc.ref_sumsq(p0, np.float32), abs(ref), "sgd_sumsq", tag)
    assert g.untouched()


# ----------------------------------------------------------------------------------------------------------------------
# global average pooling
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C", lc.GAP_SHAPES)
def test_global_average_pooling(B, HW, C, cuda, E):
    for kind in lc.gap_kinds(HW):
        x0, dy0, dxold = lc.gap_input(B, HW, C, kind)
        tag = "B %d HW %d C %d %s" % (B, HW, C, kind)
        x, y = dense(x0, cuda), blank(B, C, cuda, 3)
        E.call("dj_global_avg_pool_fwd", x.ptr, y.ptr, B, HW, C)
        torch.cuda.synchronize()
        if kind == "dyadic":
            assert_exact(y.result(), lc.ref_gap_fwd(x0), "y " + tag)
        else:
            within(y.result(), lc.ref_gap_fwd(x0), lc.ref_gap_fwd(x0, F32), lc.gap_fwd_scale(x0), "gap", "y " + tag)
        dy = dense(dy0, cuda, 2)
        for beta in lc.GAP_BETA:
            dx = dense(dxold, cuda, 3) if beta else blank(B * HW, C, cuda, 3)
            E.call("dj_global_avg_pool_bwd", dy.ptr, dx.ptr, B, HW, C, beta)
            torch.cuda.synchronize()
            ref = lc.ref_gap_bwd(dy0, HW, dxold, beta).reshape(B * HW, C)
            if kind == "dyadic":
                assert_exact(dx.result(), ref, "dx beta %d %s" % (beta, tag))
            else:
                within(dx.result(), ref, lc.ref_gap_bwd(dy0, HW, dxold, beta, np.float32).reshape(B * HW, C),
                       lc.gap_bwd_scale(dy0, HW, dxold, beta).reshape(B * HW, C), "gap", "dx beta %d %s" % (beta, tag))
        assert untouched(x, dy)
