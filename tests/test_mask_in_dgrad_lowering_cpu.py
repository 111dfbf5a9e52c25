"""Structure of the training plan with the ReLU mask of the block outputs in the input-gradient GEMMs (keras/layers.py
`_relu_mask_in_dgrad`), lowered on the host (nothing runs): which layers get the masked launch, that the knob switches it
off, and that the plan-time checks on the shared gradient buffers hold for the whole SSD300 graph."""
import pytest
import torch


def _lower(monkeypatch, knob, batch=2):
    from jpeg_detection_resnet_ssd_amd import workloads
    monkeypatch.setenv("DJ_MASK_IN_DGRAD", knob)
    monkeypatch.setenv("DJ_AUTOTUNE", "table")
    model, _ = workloads.build_ssd("deconv", weight_seed=42)
    model._ensure_params(device=torch.device("cpu"))
    return model, model._plan(batch, True, True)


def test_ssd_plan_masks_block_output_gradients_where_it_may(monkeypatch):
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    model, plan = _lower(monkeypatch, "1")
    masked = set(plan.masked_dgrads)
    assert len(masked) >= 8, sorted(masked)
    by_name = {l.name: l for l in model.layers}
    for name in masked:
        lyr = by_name[name]
        # the first 1x1 stride-1 convolution of a bottleneck block, reading the ReLU-ed sum of the block before it
        assert isinstance(lyr, L.Conv2D) and lyr.kernel_size == (1, 1) and lyr.strides == (1, 1) and name.endswith("_branch2a")
        src = lyr.inbound[0].layer
        assert isinstance(src, L.Activation) and isinstance(src.inbound[0].layer, L.Add)
        x = plan.values[id(lyr.inbound[0])]
        assert x.grad.premasked and x.add_relu_first is lyr
    # a block whose first convolution is strided (stage transitions) keeps the plain path
    assert not any(by_name[n].strides != (1, 1) for n in masked)
    # identity shortcuts behind a pre-masked sum share the gradient buffer of that sum
    shared = 0
    for lyr in model.layers:
        if isinstance(lyr, L.Add):
            out = plan.values[id(lyr.outbound[0])]
            if out.grad is not None and out.grad.premasked:
                for t in lyr.inbound:
                    v = plan.values[id(t)]
                    if not v.is_affine and v.grad is not None and v.grad.buf.data_ptr() == out.grad.buf.data_ptr():
                        shared += 1
                        assert all(r.consumed for r in v.grad.alias_readers) and len(v.grad.alias_readers) == 1
    assert shared >= 4, shared
    _, plain = _lower(monkeypatch, "0")
    assert plain.masked_dgrads == []


def test_a_masked_gradient_takes_no_further_writer():
    from jpeg_detection_resnet_ssd_amd.engine import GradRef, Plan, Value
    plan = Plan(torch.device("cpu"), 1, False)
    v = Value(torch.zeros(1, 2, 2, 4), needs_grad=True, name="v")
    buf, beta = plan.grad_of(v)
    assert beta == 0 and plan.grad_of(v)[1] == 1
    v.grad.premasked = True
    with pytest.raises(AssertionError, match="masked by its last writer"):
        plan.grad_of(v)
    # a shared buffer may only be written once every reader of its previous contents has been emitted
    w = Value(torch.zeros(1, 2, 2, 4), needs_grad=True, name="w")
    reader = GradRef(buf)
    plan.alias_grad(w, buf, [reader])
    with pytest.raises(AssertionError, match="overwritten before a reader"):
        plan.grad_of(w)
    reader.consumed = True
    assert plan.grad_of(w)[1] == 1 and plan.grad_of(w)[0] is buf


def test_lowering_state_of_values_and_gradrefs_is_declared():
    """The lowerings keep their per-tensor state in declared attributes of Value / GradRef: a fresh Value reads the
    neutral value for each (a fusion is off until a lowering switches it on) and a name that is not declared -- a
    misspelt one would silently switch a fusion off -- raises where it is assigned."""
    from jpeg_detection_resnet_ssd_amd.engine import GradRef, Value
    v = Value(torch.zeros(1, 2, 2, 4), needs_grad=True, name="v")
    for name in ("grad", "alias_of", "alias_view", "pad", "conv_stats", "relu_child", "bn", "bn_saved", "bn_parent", "_mat",
                 "add_relu_first", "pending_add", "ready_event", "side_done"):
        assert getattr(v, name) is None, name
    for name in ("bn_applies_mask", "constant"):
        assert getattr(v, name) is False, name
    g = GradRef(v.buf)
    assert g.mask_y is None and g.also is None and g.bwd_partial is None and g.alias_readers == ()
    assert g.premasked is False and g.consumed is False
    for obj in (v, g):
        with pytest.raises(AttributeError):
            obj.bn_svaed = (None, None)
        assert not hasattr(obj, "__dict__")
