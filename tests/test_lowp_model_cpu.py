"""Premises of tests/test_lowp_model_gpu.py, checked without a GPU over the tables of tests/lowp_model_cases.py:
(a) the grid makes the fp32 prologue exact; (b) the model and the unrounded oracle lie at least 50 bounds apart, so the
GPU test can tell them apart; (c) a torch fp32 convolution of the rounded operands -- fp32 accumulation of exact products
in an order of its own -- meets both GPU bounds; (d) every perturbed model (truncation, one operand unrounded, fp16 / bf16
swapped, prologue after the rounding, statistics of the rounded result) misses the rel-L2 bound by at least 50x; (e) the
legality table is the launcher's predicates; (f) every launch form and storage combination has a case."""
import functools

import pytest
import torch

import lowp_model_cases as C
from lowp_model_cases import BF16, F16, F32

MARGIN = 50 * C.REL_L2_BOUND
ROUNDING_GEOMS = [g.name for g in C.GEOMS if g.name != "fallback"]


def _legal_storages(mode, name, direction, form):
    for g, d, f, sname, types, ok in C.cases(mode):
        if (g.name, d, f) == (name, direction, form) and ok:
            yield sname, types


def test_grid_prologues_are_exact_in_fp32():
    """(a) x*scale+shift, and the residual-add form, evaluated in fp32 -- as two roundings (mul, add) and as one (the
    fp64 value rounded once = what an fma gives) -- equal their fp64 values, with fp32 and with fp16 tensors; and a
    third of the values still needs a non-trivial fp16 rounding."""
    needs_rounding = []
    for g in C.GEOMS:
        o = C.operands(g.name)
        for dt in (F32, F16):
            x, r = C.stored(o["xg"], dt).float(), C.stored(o["res"], dt).float()
            exact = x.double() * o["sc"].double() + o["sh"].double()
            assert torch.equal((x * o["sc"] + o["sh"]).double(), exact) and torch.equal(exact.float().double(), exact)
            exact3 = exact + r.double() * o["rsc"].double() + o["rsh"].double()
            two_step = (x * o["sc"] + o["sh"]) + (r * o["rsc"] + o["rsh"])
            assert torch.equal(two_step.double(), exact3) and torch.equal(exact3.float().double(), exact3)
            needs_rounding.append(float((C.model_round(exact3.float(), F16) != exact3).double().mean()))
        # the BatchNormalization-backward epilogue: fp16 holds z itself, mask argument and x-hat are exact
        z = o["z"]
        assert torch.equal(z.to(F16).float(), z)
        m = z.double() * o["sc"].double() + o["sh"].double()
        xh = (z.double() - o["mean"].double()) * o["invstd"].double()
        assert torch.equal((z * o["sc"] + o["sh"]).double(), m) and torch.equal(((z - o["mean"]) * o["invstd"]).double(), xh)
    assert min(needs_rounding) >= 0.3, needs_rounding


@functools.lru_cache(maxsize=None)
def _fp32_emulation(name, mode, direction, form, types):
    """torch fp32 arithmetic on the rounded operands, through the same launch-form algebra as the model."""
    g, o = C.GEOM[name], C.operands(name)
    ref = C.REFS[direction](name, mode, form, types)
    T = C.arith_type(mode, direction) if C.branch_free(g, direction, form == "transpose_bias") else None
    f = lambda t: C.model_round(t, T).float()
    if direction == "fwd":
        x_dt = types[0]
        if form == "plain_bias_relu":
            a = C.stored(o["x"], x_dt).float()
        elif form == "addrelu_sum":
            a = C.pro_addrelu(C.stored(o["xg"], x_dt), o["sc"], o["sh"], C.stored(o["res"], x_dt), o["rsc"], o["rsh"]).float()
        else:
            a = C.pro_affine(C.stored(o["xg"], x_dt), o["sc"], o["sh"]).float()
        y = C.conv(g, f(a), f(o["w"]))
        got = torch.relu(y + o["bias_co"]) if form == "plain_bias_relu" else y
        return ref, got, y
    if direction == "dgrad":
        x0 = torch.zeros(g.b, g.h, g.w, g.ci, requires_grad=True)
        C.conv(g, x0, f(o["w"])).backward(f(C.stored(o["dy"], types[0]).float()))
        y = x0.grad
        got = y + o["bias_ci"] if form == "transpose_bias" else y + C.stored(o["prev"], types[2]).float() if form == "beta" else y
        return ref, got, y
    a = C.stored(o["x"], types[0]).float() if form == "plain" else C.pro_affine(C.stored(o["xg"], types[0]), o["sc"], o["sh"]).float()
    w0 = torch.zeros(g.k, g.k, g.ci, g.co, requires_grad=True)
    C.conv(g, f(a), w0).backward(f(C.stored(o["dy"], types[1]).float()))
    return ref, w0.grad, w0.grad


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("name", ROUNDING_GEOMS)
def test_model_is_far_from_the_unrounded_oracle_and_fp32_accumulation_meets_the_bounds(name, mode):
    """(b) and (c), every direction and form of a geometry, with fp32 tensors and with the first legal 16-bit combination
    (in mode bfloat16 there is none)."""
    g = C.GEOM[name]
    for direction, forms in C.FORMS.items():
        for form in forms:
            if not C.form_applies(g, direction, form):
                continue
            for sname, types in list(_legal_storages(mode, name, direction, form))[:2]:
                ref, got, y = _fp32_emulation(name, mode, direction, form, types)
                tag = (direction, form, sname)
                if C.branch_free(g, direction, form == "transpose_bias"):
                    plain = C.gemm_model(g, direction, *_operands_of(name, direction, form, types), None)[0]
                    assert C.rel_l2(ref.extra.get("y", ref.pre).reshape(plain.shape), plain) >= MARGIN, tag      # (b)
                rel, ratio = C.check_f32(got, ref)                                                              # (c)
                assert C.passes_f32(rel, ratio), (tag, rel, ratio)
                out_dt = types[2] if direction != "wgrad" else F32
                if out_dt != F32:
                    bad, straddle = C.check_16(got.to(out_dt), ref, out_dt)
                    assert bad == 0, (tag, bad, straddle)
                if form == "bn_stats":
                    (s1, b1), (s2, b2) = C.stats_model(ref.extra["y"], ref.extra["S2"], ref.K)
                    yy = y.reshape(-1, g.co)
                    assert bool(((yy.sum(0).double() - s1).abs() <= b1).all()), tag
                    assert bool((((yy * yy).sum(0).double() - s2).abs() <= b2).all()), tag
                    assert C.rel_l2(yy.sum(0), s1) <= C.REL_L2_BOUND and C.rel_l2((yy * yy).sum(0), s2) <= 2 * C.REL_L2_BOUND, tag


def _operands_of(name, direction, form, types):
    """(a, b) of the GEMM as fp64 values before the operand rounding."""
    o = C.operands(name)
    if direction == "dgrad":
        return C.stored(o["dy"], types[0]).double(), o["w"]
    if direction == "wgrad":
        a = C.stored(o["x"], types[0]).double() if form == "plain" else C.pro_affine(C.stored(o["xg"], types[0]), o["sc"], o["sh"])
        return a, C.stored(o["dy"], types[1]).double()
    if form == "plain_bias_relu":
        return C.stored(o["x"], types[0]).double(), o["w"]
    if form == "addrelu_sum":
        return C.pro_addrelu(C.stored(o["xg"], types[0]), o["sc"], o["sh"], C.stored(o["res"], types[0]), o["rsc"], o["rsh"]), o["w"]
    return C.pro_affine(C.stored(o["xg"], types[0]), o["sc"], o["sh"]), o["w"]


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("variant", C.PERTURBATIONS)
def test_perturbed_models_miss_the_bound_by_50x(variant, mode):
    """(d) on the forms without additions behind the GEMM (a bias or an accumulated tensor only dilutes the distance)."""
    for name in ("map7x5", "pointwise", "c96"):
        g = C.GEOM[name]
        if variant == "stats_rounded":
            continue          # test_statistics_of_the_rounded_result_are_told_apart
        for direction, form in (("fwd", "bn_stats"), ("fwd", "addrelu_sum"), ("dgrad", "plain"), ("wgrad", "pro"), ("wgrad", "plain")):
            if not C.form_applies(g, direction, form) or (variant == "pro_after" and form in ("plain",)):
                continue
            types = C.STORAGE[direction][0][1]
            ref = C.REFS[direction](name, mode, form, types)
            bad = C.REFS[direction](name, mode, form, types, variant=variant)
            assert C.rel_l2(bad.result, ref.result) >= MARGIN, (name, direction, form, C.rel_l2(bad.result, ref.result))


def test_statistics_of_the_rounded_result_are_told_apart():
    """(d), last item: column totals taken from the ROUNDED stored result instead of the fp32 accumulators (mode float16:
    only there is a result held in 16 bits).  The rigorous column bound of the GPU test cannot see this -- it is u K
    sum|a||b|, far above one fp16 rounding of y averaged over a column -- so the GPU test also holds the totals to the
    rel-L2 bound of the results themselves (sums 2e-6, squares twice that), and that is what is measured here.
    bf16 input gradients (the BatchNormalization-backward sums): >= 50 bounds at every geometry (measured 1.5e-3 .. 2e-3).
    fp16 forward results: the roundings of a column's rows average out, sums 2.1e-5 .. 1.6e-4 and squares 4.2e-5 .. 2.7e-4:
    >= 50 bounds on the maps of a few rows (map1x1, strided1x1_c48), >= 10 bounds everywhere."""
    mode, fwd_margins = "float16", {}
    for g in C.GEOMS:
        if C.branch_free(g, "fwd"):
            ref = C.forward_ref(g.name, mode, "bn_stats", (F16, F32, F16))
            (s1, _), (s2, _) = C.stats_model(ref.extra["y"], ref.extra["S2"], ref.K)
            yr = C.model_round(ref.extra["y"].float(), F16)
            fwd_margins[g.name] = min(C.rel_l2(yr.sum(0), s1) / C.REL_L2_BOUND, C.rel_l2((yr * yr).sum(0), s2) / (2 * C.REL_L2_BOUND))
        if C.branch_free(g, "dgrad") and C.form_applies(g, "dgrad", "bnb_masked"):
            d = C.dgrad_ref(g.name, mode, "bnb_masked", (BF16, F32, BF16))
            yr = C.model_round(d.extra["y"].float(), BF16)
            for wname, rounds in (("mask", False), ("xhat", True)):
                tot, _ = C.weighted_sum_model(d.extra["y"], d.extra["S2"], d.K, d.extra[wname], rounds)
                assert C.rel_l2((yr * d.extra[wname]).sum(0), tot) >= MARGIN, (g.name, wname)
    assert min(fwd_margins.values()) >= 10 and fwd_margins["map1x1"] >= 50 and fwd_margins["strided1x1_c48"] >= 50, fwd_margins


def test_legality_table_is_the_launchers_predicate():
    """(e) include/dj_hip.h: 16-bit tensors in arithmetic mode 1 only, on the branch-free kernel's preconditions --
    restated here from the numbers alone (dj_conv_launch.h fast_mode), independently of lowp_model_cases.branch_free."""
    def fast_mode(am, bmd, srcC, N, ldb, sH):
        if am != 2 and srcC % 32:
            return False
        if am == 1 and sH != 1:
            return False
        if am == 2 and srcC % 4:
            return False
        if bmd == 0 and (N % 4 or ldb % 4):
            return False
        return not (bmd == 1 and srcC % 32)

    seen = set()
    for mode in C.MODES:
        for g, direction, form, sname, types, ok in C.cases(mode):
            if direction == "fwd":
                fast = fast_mode(0, 0, g.ci, g.co, g.co, g.s) and g.ci % 4 == 0 and g.co % 4 == 0
            elif direction == "wgrad":
                fast = fast_mode(2, 0, g.ci, g.co, g.co, g.s) and g.ci % 4 == 0 and g.co % 4 == 0
            elif g.k == 1 and g.s > 1 and form != "transpose_bias":
                fast = fast_mode(0, 1, g.co, g.ci, g.co, 1) and g.co % 4 == 0
            else:
                fast = fast_mode(1, 1, g.co, g.ci, g.co, g.s) and g.co % 4 == 0
            want = all(t == F32 for t in types) or (mode == "float16" and fast)
            assert ok == want, (mode, g.name, direction, form, sname)
            seen.add((direction, ok))
            # storage types the entry points take at all: fp16 activations, bf16 gradients, the shadow of the direction
            allowed = {"fwd": (F16, F16, F16), "dgrad": (BF16, BF16, BF16), "wgrad": (F16, BF16)}[direction]
            assert all(t in (F32, a) for t, a in zip(types, allowed))
    assert seen == {(d, ok) for d in C.FORMS for ok in (True, False)}      # every direction is both taken and refused
    # the one off-precondition geometry computes the unrounded oracle in every direction
    fb = C.GEOM["fallback"]
    assert not any(C.branch_free(fb, d, b) for d in C.FORMS for b in (False, True))


def test_every_form_and_storage_combination_has_a_case():
    """(f) ... a LEGAL case in mode float16, and a fp32-tensor case in mode bfloat16; both K-step depths, an M off the
    tile, the asymmetric `same`, and no geometry above 2 x 12 x 12 x 256."""
    legal16 = {(d, f, s) for g, d, f, s, t, ok in C.cases("float16") if ok}
    for direction, forms in C.FORMS.items():
        for form in forms:
            for sname, types in C.STORAGE[direction]:
                if form in ("slabs", "atomics") and types[2] != F32:
                    continue
                assert (direction, form, sname) in legal16, (direction, form, sname)
            assert any((d, f, s) == (direction, form, "f32") and ok for g, d, f, s, t, ok in C.cases("bfloat16"))
    on = [g for g in C.GEOMS if C.branch_free(g, "fwd")]
    assert any(g.ci % 64 == 0 for g in on) and any(g.ci % 64 for g in on)
    assert any(g.co % 64 == 0 for g in on) and any(g.co % 64 for g in on if C.branch_free(g, "dgrad"))
    assert any((g.b * C.out_size(g)[0] * C.out_size(g)[1]) % 64 for g in on)
    assert any(g.k == 2 and g.pad == "same" and C.pads(g) == (0, 0) for g in on)
    assert all(g.b * g.h * g.w * max(g.ci, g.co) <= 2 * 12 * 12 * 256 for g in C.GEOMS)
    assert len({g.name for g in C.GEOMS}) == len(C.GEOMS)
