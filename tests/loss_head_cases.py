"""Cases shared by tests/test_loss_head_cases_cpu.py and tests/test_loss_head_gpu.py: the code paths of csrc/dj_loss.hip
(softmax, the SSD multibox loss with batch-wide hard-negative mining, categorical cross-entropy, global average pooling) and
of the Keras SGD update (a rule of csrc/dj_optim.hip), the inputs that reach them and plain float64 references.

No GPU is imported here.  Every output operand is a `Slab` (tests/norm_edge_cases.py): a view inside a wider buffer filled
with one quiet-NaN bit pattern, so that everything around an output can be compared bit for bit after a launch.

Tolerances.  A result that is exact by construction (dyadic data: multiples of 1/8 with power-of-two scalars; every zero;
counts; the keep set) must EQUAL the float64 reference cast to fp32.  Everywhere else the bound comes from the reference
alone: the same formula is evaluated on the CPU in fp32 and in float64 on the same inputs, both errors are normalised by the
same per-element `scale` (stated at each reference: |ref|, the largest |ref| of the row, or the sum of the absolute terms
where terms cancel), and

    bound = max(MARGIN * max_elements(|fp32 - float64| / scale), FLOOR),   MARGIN = 8, FLOOR = 2^-21 (4 ulp, relative)

The margin covers a different summation order and the 1-2 ulp device expf, logf and division against the host's.  An element
whose scale is zero must be matched exactly.  The sum of squares of the SGD update is accumulated with atomics; its fp32
evaluation is numpy's pairwise sum.
"""
import collections
import functools
import itertools

import numpy as np
import torch

from norm_edge_cases import SENTINEL_BITS, Slab, dyadic, f64, rng_for   # noqa: F401 (re-exported to the two test files)
from optimizer_cases import several_passes
from oracle import keras_ops as ko

MARGIN = 8.0
FLOOR = 2.0 ** -21

# --------------------------------------------------------------------------------------------------------------------
# launcher rules, copied from csrc/dj_loss.hip (SGD_GROUPS_PER_PASS: from csrc/dj_optim.hip)
# --------------------------------------------------------------------------------------------------------------------
EW_BLOCK_CAP = 4096      # ew_blocks: workgroups of 256 threads of the grid-stride kernels (GAP, the SSD backward)
SGD_GROUPS_PER_PASS = 2048 * 256     # dj_optim_groups_per_pass(): threads of the capped grid, each a group of four elements
LOSS_BLOCKS = 512        # DJ_LOSS_BLOCKS: the per-box pass
MINE_BLOCKS = 256        # DJ_MINE_BLOCKS: the histogram and mark kernels
DJ_HB = 2048             # bins of a histogram level (levels 0 and 1; level 2 uses 1024 of them)
THREADS = 256


def softmax_group(C):
    g = 8
    while g < 64 and g < C:
        g <<= 1
    return g


def softmax_rows_per_block(C):
    """Four waves of 64 / G rows each."""
    return 4 * (64 // softmax_group(C))


def ew_blocks(total):
    return min(max(-(-total // THREADS), 1), EW_BLOCK_CAP)


def loss_blocks(nbox):
    return min(ew_blocks(nbox), LOSS_BLOCKS)


def mine_blocks(nbox):
    return min(ew_blocks(nbox), MINE_BLOCKS)


def ssd_workspace_floats(nbox):
    return 5 * nbox + 4 * LOSS_BLOCKS + MINE_BLOCKS + 3 * DJ_HB + 8 + 8


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.int64)


def bits1(v):
    return int(bits_of(v).reshape(-1)[0])


def scan_position(bits, level):
    """mine_scan_level: -> (thread, position inside the thread's run, length of the run) of the bin that the fp32 pattern
    `bits` falls into at `level` (11 + 11 + 10 bits; the scan runs from the top bin down, nbins / 256 bins per thread)."""
    field = (bits >> 21) & 2047 if level == 0 else ((bits >> 10) & 2047 if level == 1 else bits & 1023)
    per = (1024 if level == 2 else DJ_HB) // THREADS
    j = (1024 if level == 2 else DJ_HB) - 1 - field
    return j // per, j % per, per


# --------------------------------------------------------------------------------------------------------------------
# the bound
# --------------------------------------------------------------------------------------------------------------------
def rel_err(got, ref, scale):
    """max over the elements of |got - ref| / scale; an element with scale 0 counts 0 if it is matched exactly, inf if not."""
    ref = f64(ref)
    diff = np.abs(f64(got).reshape(ref.shape) - ref)
    scale = np.broadcast_to(f64(scale), ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.inf))
    return float(r.max()) if r.size else 0.0


def bound(ref32, ref64, scale):
    return max(MARGIN * rel_err(ref32, ref64, scale), FLOOR)


def row_max(a):
    return np.abs(f64(a)).max(axis=-1, keepdims=True)


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# --------------------------------------------------------------------------------------------------------------------
# softmax
# --------------------------------------------------------------------------------------------------------------------
SOFTMAX_C = [1, 7, 8, 9, 16, 17, 21, 32, 33, 64, 65, 130]
SOFTMAX_BIG_C = [7, 16, 21, 130]          # one C per group size 8, 16, 32, 64: logits of magnitude 80
SOFTMAX_LD_EXTRA = [0, 3]                 # ld_dp = C and C + 3
SOFTMAX_BETA = [0, 1]


def softmax_rows(C):
    """One row; a block short of one row; a block and a row; three blocks and two rows: each leaves dead rows in its last
    block, and with G < 64 the last live wave holds live and dead sub-rows (but for the 26 rows of G = 32)."""
    r = softmax_rows_per_block(C)
    return [1, r - 1, r + 1, 3 * r + 2]


def softmax_input(rows, C, big=False):
    """x, dp, dx0 (fp32).  `big`: logits of -80 and +80 (a few classes each side, two apart at most) and one class at 90 --
    exp(90) overflows fp32, so the result is finite only if the row maximum is subtracted."""
    rng = rng_for("softmax", rows, C, big)
    x = rng.standard_normal((rows, C)) * 4
    if big:
        x = rng.choice([-80.0, 80.0], size=(rows, C)) + rng.uniform(-1, 1, (rows, C))
        x[np.arange(rows), rng.integers(0, C, rows)] = 90.0
    return (x.astype(np.float32), rng.standard_normal((rows, C)).astype(np.float32),
            rng.standard_normal((rows, C)).astype(np.float32))


def ref_softmax(x, dtype=torch.float64):
    """The oracle's softmax; scale: the largest value of the row."""
    return ko.softmax(T(x, dtype)).numpy()


def ref_softmax_bwd(p, dp, dx0, beta, dtype=np.float64):
    """dx (+)= p * (dp - sum(dp * p)) on the GIVEN fp32 probabilities; scale: softmax_bwd_scale."""
    p, dp = np.asarray(p, dtype=dtype), np.asarray(dp, dtype=dtype)
    dot = (p * dp).sum(axis=-1, keepdims=True, dtype=dtype)
    v = p * (dp - dot)
    return v + np.asarray(dx0, dtype=dtype) if beta else v


def softmax_bwd_scale(p, dp, dx0, beta):
    """The terms p*dp and p*sum(dp*p) cancel in a saturated row: the largest |p| times the largest |dp| of the row, plus
    the largest old |dx| where it is accumulated."""
    return row_max(p) * row_max(dp) + (row_max(dx0) if beta else 0.0)


# --------------------------------------------------------------------------------------------------------------------
# global average pooling
# --------------------------------------------------------------------------------------------------------------------
GAP_SHAPES = [(1, 1, 1), (2, 49, 30), (3, 64, 128), (2, 2, 524289)]     # the last: B*C and B*HW*C > 4096*256
GAP_BETA = [0, 1]


def gap_kinds(HW):
    return ["dyadic", "normal"] if HW & (HW - 1) == 0 else ["normal"]


def gap_input(B, HW, C, kind):
    rng = rng_for("gap", B, HW, C, kind)
    if kind == "dyadic":
        return dyadic(rng, (B, HW, C)), dyadic(rng, (B, C)), dyadic(rng, (B, HW, C))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(B, HW, C), f(B, C), f(B, HW, C)


def ref_gap_fwd(x, dtype=torch.float64):
    """The oracle's mean over H and W (HW as H, W = 1); scale: the mean of |x|."""
    B, HW, C = x.shape
    return ko.global_average_pooling(T(x, dtype).reshape(B, HW, 1, C)).numpy()


def gap_fwd_scale(x):
    return np.abs(f64(x)).mean(axis=1)


def ref_gap_bwd(dy, HW, dx0, beta, dtype=np.float64):
    """dx (+)= dy / HW at every pixel; scale: |dy| / HW plus the old |dx|."""
    dy = np.asarray(dy, dtype=dtype)
    v = np.repeat((dy / dtype(HW))[:, None, :], HW, axis=1)
    return v + np.asarray(dx0, dtype=dtype) if beta else v


def gap_bwd_scale(dy, HW, dx0, beta):
    v = np.repeat((np.abs(f64(dy)) / HW)[:, None, :], HW, axis=1)
    return v + np.abs(f64(dx0)) if beta else v


# --------------------------------------------------------------------------------------------------------------------
# SGD
# --------------------------------------------------------------------------------------------------------------------
SGD_N = [1, 63, 257, several_passes(SGD_GROUPS_PER_PASS)]
SGD_SUMSQ0 = 3.5
# lr_t, momentum values, l2 values, grad_scale values; the dyadic ones are powers of two
SGD_SCALARS = {"dyadic": (0.25, (0.0, 0.5), (0.0, 0.25), (1.0, 0.125)),
               "normal": (0.1 / (1 + 1e-4 * 7), (0.0, 0.9), (0.0, 5e-4), (1.0, 0.125))}
SgdCfg = collections.namedtuple("SgdCfg", "lr_t momentum nesterov l2 grad_scale sumsq")


def sgd_configs(n, kind):
    """Every combination of nesterov, sumsq given / null, momentum, l2 and grad_scale; past the grid (more groups of four
    than SGD_GROUPS_PER_PASS) six of them, in which every value of every parameter occurs with both values of nesterov."""
    lr_t, moms, l2s, gss = SGD_SCALARS[kind]
    if sgd_groups(n) <= SGD_GROUPS_PER_PASS:
        picks = itertools.product((0, 1), (True, False), (0, 1), (0, 1), (0, 1))
    else:   # nesterov, sumsq, index of momentum, of l2, of grad_scale
        picks = [(0, True, 1, 1, 1), (0, False, 0, 0, 0), (0, True, 0, 1, 0), (1, True, 1, 0, 1), (1, False, 0, 1, 0),
                 (1, True, 0, 0, 1)]
    return [SgdCfg(lr_t, moms[a], nes, l2s[b], gss[c], ss) for nes, ss, a, b, c in picks]


def sgd_groups(n):
    """One thread per group of four consecutive elements."""
    return (n + 3) // 4


def sgd_input(n, kind):
    rng = rng_for("sgd", n, kind)
    if kind == "dyadic":
        return dyadic(rng, n), dyadic(rng, n), dyadic(rng, n)
    return tuple(rng.standard_normal(n).astype(np.float32) for _ in range(3))


def f32val(v):
    """A scalar as the kernel receives it: rounded to fp32."""
    return float(np.float32(v))


def ref_sgd(p, g, v, cfg, dtype=torch.float64):
    """g' = g*grad_scale + 2*l2*p, then the oracle's Keras step with lr_t as given.  -> (new p, new v)."""
    pt, gt, vt = T(p, dtype), T(g, dtype), T(v, dtype)
    g_eff = gt * f32val(cfg.grad_scale) + 2.0 * f32val(cfg.l2) * pt
    new_p, new_v = ko.sgd_keras_step(pt, g_eff, vt, f32val(cfg.lr_t), f32val(cfg.momentum), 0.0, 0, bool(cfg.nesterov))
    return new_p.numpy(), new_v.numpy()


def sgd_scales(p, g, v, cfg):
    """Sums of the absolute terms of new v and of new p."""
    p, g, v = np.abs(f64(p)), np.abs(f64(g)), np.abs(f64(v))
    lg = f32val(cfg.lr_t) * (g * f32val(cfg.grad_scale) + 2.0 * f32val(cfg.l2) * p)
    sv = f32val(cfg.momentum) * v + lg
    return p + (f32val(cfg.momentum) * sv + lg if cfg.nesterov else sv), sv


def ref_sumsq(p, dtype=np.float64):
    """SGD_SUMSQ0 + sum(p^2) of the pre-update p; in fp32 numpy's pairwise sum.  scale: |ref|."""
    p = np.asarray(p, dtype=dtype)
    return dtype(SGD_SUMSQ0) + (p * p).sum(dtype=dtype)


# --------------------------------------------------------------------------------------------------------------------
# categorical cross-entropy
# --------------------------------------------------------------------------------------------------------------------
CCE_SHAPES = [(1, 1), (3, 5), (5, 64), (6, 65), (9, 1000)]
CCE_LABELS = ["onehot", "soft"]
CCE_UPSTREAM = [1.0, -2.0]
CCE_TINY_ROW, CCE_ONE_ROW = 0, 1          # one-hot labels, rows >= 3: q = 1e-9 and q = 1 at the labelled class


def cce_variants():
    """(labels, scaled, d_probs given, upstream)"""
    return list(itertools.product(CCE_LABELS, (False, True), (True, False), CCE_UPSTREAM))


def cce_input(rows, C, labels, scaled):
    """y_true, probs (fp32).  The probabilities are a softmax of unit-variance logits (none anywhere near 1e-7), times a
    per-row factor in [0.25, 4] if `scaled`.  With one-hot labels and rows >= 3, row 0 has q = 1e-9 at its labelled class
    and row 1 is that class alone (q = 1): both are clipped, their gradient rows are zero."""
    rng = rng_for("cce", rows, C)
    probs = ref_softmax(rng.standard_normal((rows, C)))
    lab = rng.integers(0, C, rows)
    y = np.zeros((rows, C))
    if labels == "onehot":
        y[np.arange(rows), lab] = 1.0
        if rows >= 3:
            probs[CCE_TINY_ROW, lab[CCE_TINY_ROW]] = 0.0
            probs[CCE_TINY_ROW, lab[CCE_TINY_ROW]] = 1e-9 * probs[CCE_TINY_ROW].sum()
            probs[CCE_ONE_ROW] = 0.0
            probs[CCE_ONE_ROW, lab[CCE_ONE_ROW]] = 1.0
    else:
        y[:] = 0.1 / max(C - 1, 1)
        y[np.arange(rows), lab] = 0.9
    if scaled:
        probs = probs * rng.uniform(0.25, 4.0, (rows, 1))
    return y.astype(np.float32), probs.astype(np.float32), lab


def cce_q(probs):
    probs = f64(probs)
    return probs / probs.sum(axis=-1, keepdims=True)


def ref_cce(y, probs, upstream, dtype=torch.float64):
    """The oracle's renormalise, clip and -sum(y log q), its mean, and autograd of upstream * mean with respect to probs.
    scales: the largest loss of the tensor (loss_rows), |mean|, the largest |gradient| of the row (d_probs).
    A row clipped at the top loses -log(1 - 1e-7) = 1.0e-7 in float64 and -log(1 - 2^-23) = 1.19e-7 in fp32, whose nearest
    value to 1 - 1e-7 that is: invisible beside any other row, but (1, 1) has no other row, and there the rule gives a bound
    of 8 * 19 %."""
    pt = T(probs, dtype).requires_grad_(True)
    rows = ko.categorical_crossentropy(T(y, dtype), pt)
    mean = rows.mean()
    (mean * upstream).backward()
    return rows.detach().numpy(), mean.detach().numpy(), pt.grad.numpy()


# --------------------------------------------------------------------------------------------------------------------
# SSD loss: the per-box pass and the backward
# --------------------------------------------------------------------------------------------------------------------
SSD_NCLS = [2, 21, 81]
SSD_NBOX = [1, 255, 257]
SSD_ALPHA = [1.0, 0.25]
SSD_UPSTREAM = [1.0, -0.5]
# t - p of the four offsets: exactly 0, +-1, +-(1 - 2^-20), +-1.5, and multiples of 1/16 up to 3
LOC_SPECIAL = [0.0, 1.0, -1.0, 1.0 - 2.0 ** -20, -(1.0 - 2.0 ** -20), 1.5, -1.5]
SsdCase = collections.namedtuple("SsdCase", "n_cls nbox y_true y_pred loc_diff clamp_boxes")


def _ssd_fill(rng, n_cls, nbox, kind, p_neg):
    """kind: 0 negative, 1 positive, 2 neutral (all class columns of y_true zero).  p_neg: None, or class rows for the
    negatives (nbox x n_cls; rows of non-negatives are ignored)."""
    W = n_cls + 12
    probs = ref_softmax(rng.standard_normal((nbox, n_cls)) * 2)
    if p_neg is not None:
        probs = np.where((kind == 0)[:, None], p_neg, probs)
    y_true = np.zeros((nbox, W))
    y_true[kind == 0, 0] = 1.0
    pos = np.flatnonzero(kind == 1)
    true_cls = rng.integers(1, n_cls, nbox)
    y_true[pos, true_cls[pos]] = 1.0
    clamp = tuple(pos[:2]) if len(pos) >= 2 else ()
    for b, v in zip(clamp, (0.0, 1e-20)):      # the p <= 1e-15 clamp: loss -log(1e-15), no class gradient
        probs[b, true_cls[b]] = v
    loc_p = rng.integers(-32, 33, (nbox, 4)) / 8.0
    d = rng.integers(-48, 49, (nbox, 4)) / 16.0
    special = rng.random((nbox, 4)) < 0.6
    d[special] = rng.choice(LOC_SPECIAL, size=int(special.sum()))
    d.reshape(-1)[:len(LOC_SPECIAL)] = LOC_SPECIAL[:min(len(LOC_SPECIAL), 4 * nbox)]
    y_true[:, n_cls:n_cls + 4] = loc_p + d
    y_true[:, n_cls + 4:] = rng.random((nbox, 8))
    y_pred = np.concatenate([probs, loc_p, rng.random((nbox, 8))], axis=1)
    return SsdCase(n_cls, nbox, y_true.astype(np.float32), y_pred.astype(np.float32), d, clamp)


@functools.lru_cache(maxsize=None)
def ssd_case(n_cls, nbox):
    """A tenth positives (box 0 among them), a tenth neutral, the rest negatives, three of them with p[0] == 1 (loss 0)."""
    rng = rng_for("ssd", n_cls, nbox)
    i = np.arange(nbox)
    kind = np.where(i % 10 == 0, 1, np.where(i % 10 == 3, 2, 0))
    p_neg = ref_softmax(rng.standard_normal((nbox, n_cls)) * 2)
    p_neg[i % 80 == 9] = np.eye(n_cls)[0]
    return _ssd_fill(rng, n_cls, nbox, kind, p_neg)


def ssd_parts(y_true, y_pred, dtype=torch.float64):
    """The oracle's per-box terms.  scales: |ref| (every one is a sum of terms of one sign)."""
    yt, yp = T(y_true, dtype), T(y_pred, dtype)
    cls = ko.log_loss(yt[:, :-12], yp[:, :-12])
    loc = ko.smooth_l1(yt[:, -12:-8], yp[:, -12:-8])
    pos = yt[:, 1:-12].max(dim=-1).values
    neg = yt[:, 0]
    return dict(cls=cls.numpy(), loc=loc.numpy(), pos=pos.numpy(), neg=neg.numpy(), negloss=(cls * neg).numpy())


def expected_k(n_pos, ratio, n_neg_min, nnz):
    return min(max(ratio * int(n_pos), n_neg_min), int(nnz))


def ssd_loss_with_keep(parts, keep, alpha):
    """(out[0], out[3], out[4]) of SSDLoss with the GIVEN keep set, in the dtype of `parts`.  scale: |ref|."""
    dt = parts["cls"].dtype.type
    keep = np.asarray(keep, dtype=dt)
    denom = max(parts["pos"].sum(dtype=dt), dt(1))
    clsp = (parts["cls"] * parts["pos"]).sum(dtype=dt) + (parts["cls"] * keep).sum(dtype=dt)
    locp = (parts["loc"] * parts["pos"]).sum(dtype=dt)
    return (clsp + dt(alpha) * locp) / denom, clsp / denom, locp / denom


def ssd_grad_with_keep(y_true, y_pred, keep, alpha, upstream, dtype=torch.float64):
    """Autograd of upstream * loss through the oracle's log_loss and smooth_l1 with the GIVEN keep set.  scale: |ref|."""
    yt, yp = T(y_true, dtype), T(y_pred, dtype).requires_grad_(True)
    cls = ko.log_loss(yt[:, :-12], yp[:, :-12])
    loc = ko.smooth_l1(yt[:, -12:-8], yp[:, -12:-8])
    pos = yt[:, 1:-12].max(dim=-1).values
    total = ((cls * pos).sum() + (cls * T(keep, dtype)).sum() + f32val(alpha) * (loc * pos).sum()) \
        / torch.clamp_min(pos.sum(), 1.0)
    (total * f32val(upstream)).backward()
    return yp.grad.numpy()


def check_keep(negloss, keep, k):
    """The keep set against the fp32 losses the selection ran on: min(k, nnz) kept, everything above the k-th largest value,
    nothing below it, of the values equal to it exactly the remainder, and never a zero loss.  -> number kept."""
    s = np.asarray(negloss, dtype=np.float32).reshape(-1)
    kept = np.asarray(keep).reshape(-1) != 0
    assert set(np.unique(np.asarray(keep))) <= {0.0, 1.0}
    kk = min(int(k), int((s != 0).sum()))
    assert int(kept.sum()) == kk, "kept %d, expected %d" % (kept.sum(), kk)
    if kk == 0:
        return 0
    thr = np.sort(s)[::-1][kk - 1]
    assert thr > 0 and not kept[s == 0].any(), "a zero-loss negative was kept"
    assert kept[s > thr].all(), "an element above the threshold was left out"
    assert not kept[s < thr].any(), "an element below the threshold was kept"
    assert int(kept[s == thr].sum()) == kk - int((s > thr).sum()), "wrong number kept among the ties at the threshold"
    return kk


# --------------------------------------------------------------------------------------------------------------------
# hard-negative mining
# --------------------------------------------------------------------------------------------------------------------
MINE_NCLS = 3
MINE_TIES = {2: 0.3, 5: 0.497, 64: 0.2}        # tie-group size -> p[0] of its bit-identical rows
MINE_ZERO_LOSS = 12
MINE_RUN = 64
MINE_RUN_START_BITS = 0x3F3173E0   # a loss just above ln 2 whose low 10 bits are 992: the run of 64 crosses a 1024 boundary
MINE_L1_EXTREME_BITS = [0x3F3FF200, 0x3F200E00]   # middle 11 bits 2044 and 3 under the cluster's top 11 bits


def p0_for_loss_bits(bits):
    """The fp32 p with -log(p) nearest to the fp32 loss pattern `bits`."""
    loss = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    return np.float32(np.exp(-np.float64(loss)))


@functools.lru_cache(maxsize=None)
def mining_case():
    """About 600 boxes, n_cls = 3; the loss of a negative is -log(p[0]).  The negatives hold
      - p[0] = 1 - 2^-m (m = 1..23), 2^-j (j = 2, 4, .., 40) and 1e-18 (clamped): losses from 2^-23 to 34.5;
      - 70 values with losses in [0.63, 0.745], inside the quarter binade [0.625, 0.75) that shares its top 11 bits, and two
        more at its ends, whose middle 11 bits are 2044 and 3 (threads 0 and 255 of the level-1 scan);
      - a run of 64 consecutive fp32 values of p[0] just below 0.5, where one step of p[0] moves the loss by one ulp: about
        32 distinct losses on either side of a multiple of 1024 ulp (they share their top 22 bits; threads 0 and 255 of the
        level-2 scan hold the last and the first of them), one of them twice;
      - tie groups of 2, 5 and 64 bit-identical rows, the 5 inside the quarter binade;
      - 12 rows with p[0] == 1: loss 0;
      - uniform p[0] for the rest;
    in a seeded random order, with 8 positives and 8 neutral boxes among them."""
    rng = rng_for("mining")
    p0 = [1.0 - 2.0 ** -m for m in range(1, 24)] + [2.0 ** -j for j in range(2, 41, 2)] + [1e-18]
    p0 += list(np.exp(-np.linspace(0.63, 0.745, 70)))
    p0 += [float(p0_for_loss_bits(b)) for b in MINE_L1_EXTREME_BITS]
    run = [p0_for_loss_bits(MINE_RUN_START_BITS)]
    for _ in range(MINE_RUN - 1):
        run.append(np.nextafter(run[-1], np.float32(0)))
    p0 += [float(v) for v in run] + [float(run[20])]
    for size, v in MINE_TIES.items():
        p0 += [v] * size
    p0 += [1.0] * MINE_ZERO_LOSS
    p0 += list(rng.uniform(0.05, 0.95, 584 - len(p0)))
    p0 = np.asarray(p0, dtype=np.float32).astype(np.float64)
    kind = np.array([0] * len(p0) + [1] * 8 + [2] * 8)
    p0 = np.concatenate([p0, np.full(16, 0.5)])
    order = rng.permutation(len(kind))
    kind, p0 = kind[order], p0[order]
    p_neg = np.stack([p0, (1 - p0) * 0.625, (1 - p0) * 0.375], axis=1)
    return _ssd_fill(rng, MINE_NCLS, len(kind), kind, p_neg)


MINE_LARGE_NBOX = 4 * 40000
MINE_LARGE_CLASSES = 7


@functools.lru_cache(maxsize=None)
def mining_large_case():
    """160000 boxes, n_cls = 21: 40 positives, some neutral boxes, some negatives with loss 0; every other negative is one
    of seven rows (box i takes row i % 7), so each tie class has members in every one of the 256 mine blocks."""
    rng = rng_for("mining_large")
    n = MINE_LARGE_NBOX
    i = np.arange(n)
    kind = np.where(i % 4001 == 5, 1, np.where(i % 97 == 3, 2, 0))
    rows = ref_softmax(rng.standard_normal((MINE_LARGE_CLASSES, 21)) * 2)
    p_neg = rows[i % MINE_LARGE_CLASSES]
    p_neg[i % 53 == 1] = np.eye(21)[0]
    return _ssd_fill(rng, 21, n, kind, p_neg)


def mining_sweep(nnz):
    """Every k the small case is asked for: 0 .. nnz + 3."""
    return range(0, nnz + 4)


def tie_class_sizes(negloss):
    """Sizes of the classes of equal non-zero losses, from the largest loss down."""
    s = np.asarray(negloss).reshape(-1)
    vals, counts = np.unique(s[s != 0], return_counts=True)
    return counts[::-1]


def mining_large_ks(negloss):
    """1, one less than a tie-class boundary, the boundary, one more, nnz (the boundary: the two largest losses)."""
    sizes = tie_class_sizes(negloss)
    b = int(sizes[0] + sizes[1])
    return [1, b - 1, b, b + 1, int(sizes.sum())]


def mining_structure(negloss):
    """What the selection can be asked on the fp32 losses `negloss`: -> dict
      top22  the largest number of distinct non-zero values that share their top 22 bits (level 2 decides among them)
      top11  the largest number of distinct values that share their top 11 bits but no two of which share their top 22
      ties   sorted sizes of the groups of equal non-zero values with more than one member
      zeros  number of zero losses;  binades  number of distinct exponents;  nnz
      scan   set of (level, thread, position, run length) of the bins of the non-zero values."""
    s = np.asarray(negloss, dtype=np.float32).reshape(-1)
    vals, counts = np.unique(s[s != 0], return_counts=True)
    b = bits_of(vals)
    top22 = max(collections.Counter((b >> 10).tolist()).values())
    top11 = max(len({v >> 10 for v in b.tolist() if v >> 21 == hi}) for hi in set((b >> 21).tolist()))
    scan = {(lv,) + tuple(int(q) for q in scan_position(int(v), lv)) for v in b.tolist() for lv in (0, 1, 2)}
    return dict(top22=top22, top11=top11, ties=sorted(int(c) for c in counts if c > 1), zeros=int((s == 0).sum()),
                binades=len(set((b >> 23).tolist())), nnz=int(counts.sum()), scan=scan)


def scan_paths(scan):
    """Names of the scan positions that REQUIRED_PATHS lists, from a `mining_structure` scan set."""
    out = set()
    for lv, t, e, per in scan:
        if e == 0:
            out.add("mine_scan_first_bin_of_run")
        if e == per - 1:
            out.add("mine_scan_last_bin_of_run")
        if t == 0:
            out.add("mine_scan_l%d_thread0" % lv)
        if t == THREADS - 1:
            out.add("mine_scan_l%d_thread255" % lv)
    return out


# n_pos == 0 and the ratio cases run on ssd_case(21, 257) (26 positives) and on its copy without positives
MINE_RATIO_CASES = [(1, 0), (1, 20), (1, 40), (3, 0), (3, 60), (3, 100)]    # (neg_pos_ratio, n_neg_min): below and above


@functools.lru_cache(maxsize=None)
def no_positive_case():
    """ssd_case(21, 257) with its positives turned into neutral boxes."""
    c = ssd_case(21, 257)
    y_true = c.y_true.copy()
    y_true[y_true[:, 1:21].max(axis=1) > 0, :21] = 0.0
    return c._replace(y_true=y_true, clamp_boxes=())


# --------------------------------------------------------------------------------------------------------------------
# the table of paths the GPU tests must reach
# --------------------------------------------------------------------------------------------------------------------
def fp32_negloss(case):
    return ssd_parts(case.y_true, case.y_pred, torch.float32)["negloss"]


def path_witnesses():
    """-> dict path name -> list of the cases that reach it, each decided by the launcher rules above."""
    w = collections.defaultdict(list)
    for C in SOFTMAX_C:
        G, rpb = softmax_group(C), softmax_rows_per_block(C)
        for rows in softmax_rows(C):
            if rows % rpb:
                w["softmax_tail_G%d" % G].append((rows, C))
            if rows % (64 // G):
                w["softmax_wave_with_live_and_dead_rows"].append((rows, C))
        if C == G:
            w["softmax_C_eq_G%d" % G].append(C)
        if C == 1:
            w["softmax_C1"].append(C)
        if C > 64 and C % G == 1:
            w["softmax_one_element_in_second_trip"].append(C)
        if any(SOFTMAX_LD_EXTRA):
            w["softmax_bwd_ld_gt_C"].append(C)
        if 1 in SOFTMAX_BETA:
            w["softmax_bwd_beta1"].append(C)
    for C in SOFTMAX_BIG_C:
        w["softmax_magnitude80_G%d" % softmax_group(C)].append(C)

    for n_cls, nbox in itertools.product(SSD_NCLS, SSD_NBOX):
        c = ssd_case(n_cls, nbox)
        w["ssd_ncls_%d" % n_cls].append(nbox)
        if nbox == 1:
            w["ssd_nbox_1"].append(n_cls)
        if 1 < nbox < THREADS:
            w["ssd_nbox_lt_256"].append((n_cls, nbox))
        if loss_blocks(nbox) > 1:
            w["ssd_two_blocks"].append((n_cls, nbox))
        if c.clamp_boxes:
            w["ssd_clamp_p"].append((n_cls, nbox))
        if (c.loc_diff == 0).any():
            w["ssd_smoothl1_zero"].append((n_cls, nbox))
        if (np.abs(c.loc_diff) == 1).any():
            w["ssd_smoothl1_one"].append((n_cls, nbox))
        parts = ssd_parts(c.y_true, c.y_pred)
        k = expected_k(parts["pos"].sum(), 3, 0, (parts["negloss"] != 0).sum())
        if ((parts["pos"] == 0) & (parts["neg"] == 0)).any() and k < (parts["neg"] != 0).sum():
            w["ssd_rows_neither_matched_nor_mined"].append((n_cls, nbox))
    if any(a != 1 for a in SSD_ALPHA):
        w["ssd_alpha"].append(SSD_ALPHA)
    if any(u != 1 for u in SSD_UPSTREAM):
        w["ssd_upstream"].append(SSD_UPSTREAM)
    if MINE_LARGE_NBOX > LOSS_BLOCKS * THREADS:
        w["ssd_loss_grid_stride"].append(MINE_LARGE_NBOX)
    if MINE_LARGE_NBOX > MINE_BLOCKS * THREADS:
        w["mine_grid_stride"].append(MINE_LARGE_NBOX)

    m = mining_structure(fp32_negloss(mining_case()))
    if m["ties"]:
        w["mine_ticket"].append(m["ties"])
    if m["top22"] >= 3:
        w["mine_level2_decides"].append(m["top22"])
    if m["top11"] >= 3:
        w["mine_level1_decides"].append(m["top11"])
    for name in scan_paths(m["scan"]):
        w[name].append("mining_case")
    sweep = mining_sweep(m["nnz"])       # k = n_neg_min, neg_pos_ratio = 0
    if any(k > 0 for k in sweep):
        w["mine_nmin"].append(sweep)
    if 1 in sweep and m["nnz"] > 1:
        w["mine_k1"].append(1)
    if m["zeros"] > 0 and m["nnz"] in sweep:
        w["mine_k_all_nonzero_with_zero_loss"].append(m["nnz"])
    if m["zeros"] > 0 and max(sweep) > m["nnz"]:
        w["mine_k_above_nnz"].append(max(sweep))
    large = fp32_negloss(mining_large_case())
    sizes = tie_class_sizes(large)
    if len(sizes) == MINE_LARGE_CLASSES and sizes.min() >= MINE_BLOCKS * THREADS // MINE_LARGE_CLASSES:
        w["mine_ticket_all_blocks"].append(sizes.tolist())
    npc = ssd_parts(no_positive_case().y_true, no_positive_case().y_pred)
    if npc["pos"].sum() == 0:
        w["mine_npos0_nmin0"].append(0)
        w["mine_npos0_nmin"].append(5)
    pc = ssd_parts(ssd_case(21, 257).y_true, ssd_case(21, 257).y_pred)
    for ratio, nmin in MINE_RATIO_CASES:
        side = "above" if nmin > ratio * pc["pos"].sum() else "below"
        if nmin < (pc["negloss"] != 0).sum():
            w["mine_ratio%d_nmin_%s" % (ratio, side)].append(nmin)

    for rows, C in CCE_SHAPES:
        if C < 64:
            w["cce_C_lt_64"].append((rows, C))
        if C > 64 and C % 64:
            w["cce_C_mod_64"].append((rows, C))
        if rows % 4:
            w["cce_rows_mod_4"].append((rows, C))
        if rows >= 3:
            y, p, lab = cce_input(rows, C, "onehot", False)
            q = cce_q(p)
            if q[CCE_TINY_ROW, lab[CCE_TINY_ROW]] < 1e-7:
                w["cce_clip_low"].append((rows, C))
            if q[CCE_ONE_ROW, lab[CCE_ONE_ROW]] > 1 - 1e-7:
                w["cce_clip_high"].append((rows, C))
    for labels, scaled, given, upstream in cce_variants():
        if not given:
            w["cce_no_dprobs"].append((labels, scaled, upstream))
        if scaled:
            w["cce_unnormalised"].append((labels, given, upstream))
        if labels == "soft":
            w["cce_soft_labels"].append((scaled, given, upstream))
        if upstream != 1:
            w["cce_upstream"].append((labels, scaled, given))

    for n in SGD_N:
        if n == 1:
            w["sgd_n1"].append(n)
        if 1 < n < 64:
            w["sgd_n_lt_64"].append(n)
        if sgd_groups(n) > SGD_GROUPS_PER_PASS:
            w["sgd_grid_stride"].append(n)
        for kind in SGD_SCALARS:
            for c in sgd_configs(n, kind):
                if not c.sumsq:
                    w["sgd_no_sumsq"].append((n, kind))
                if c.momentum == 0:
                    w["sgd_momentum0"].append((n, kind))
                if c.l2 == 0:
                    w["sgd_l2_0"].append((n, kind))

    for B, HW, C in GAP_SHAPES:
        if B * C > EW_BLOCK_CAP * THREADS:
            w["gap_fwd_grid_stride"].append((B, HW, C))
        if B * HW * C > EW_BLOCK_CAP * THREADS:
            w["gap_bwd_grid_stride"].append((B, HW, C))
        if B * HW * C == 1:
            w["gap_single_element"].append((B, HW, C))
        for beta in GAP_BETA:
            w["gap_bwd_beta%d" % beta].append((B, HW, C))
    return dict(w)


REQUIRED_PATHS = (
    ["softmax_tail_G%d" % g for g in (8, 16, 32, 64)] + ["softmax_C_eq_G%d" % g for g in (8, 16, 32, 64)]
    + ["softmax_magnitude80_G%d" % g for g in (8, 16, 32, 64)]
    + ["softmax_wave_with_live_and_dead_rows", "softmax_C1", "softmax_one_element_in_second_trip", "softmax_bwd_ld_gt_C",
       "softmax_bwd_beta1"]
    + ["mine_ticket", "mine_ticket_all_blocks", "mine_level2_decides", "mine_level1_decides", "mine_scan_first_bin_of_run",
       "mine_scan_last_bin_of_run", "mine_scan_l1_thread0", "mine_scan_l1_thread255", "mine_scan_l2_thread0",
       "mine_scan_l2_thread255", "mine_nmin", "mine_npos0_nmin0", "mine_npos0_nmin", "mine_k1",
       "mine_k_all_nonzero_with_zero_loss", "mine_k_above_nnz", "mine_grid_stride"]
    + ["mine_ratio%d_nmin_%s" % (r, s) for r in (1, 3) for s in ("below", "above")]
    + ["ssd_ncls_%d" % n for n in (2, 21, 81)]
    + ["ssd_alpha", "ssd_upstream", "ssd_clamp_p", "ssd_smoothl1_zero", "ssd_smoothl1_one",
       "ssd_rows_neither_matched_nor_mined", "ssd_nbox_1", "ssd_nbox_lt_256", "ssd_two_blocks", "ssd_loss_grid_stride"]
    + ["cce_C_lt_64", "cce_C_mod_64", "cce_rows_mod_4", "cce_no_dprobs", "cce_unnormalised", "cce_soft_labels",
       "cce_clip_low", "cce_clip_high", "cce_upstream"]
    + ["sgd_no_sumsq", "sgd_n1", "sgd_n_lt_64", "sgd_grid_stride", "sgd_momentum0", "sgd_l2_0"]
    + ["gap_bwd_beta0", "gap_bwd_beta1", "gap_fwd_grid_stride", "gap_bwd_grid_stride", "gap_single_element"]
)
