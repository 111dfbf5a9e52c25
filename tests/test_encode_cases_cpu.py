"""What tests/test_encode_gpu.py relies on, checked without a GPU: each named case of tests/encode_cases.py shows, on the
host encoder alone, the feature it is named for, under every option set; every case's host output is finite."""
import numpy as np
import pytest

import encode_cases as ec
from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.matching_utils import match_bipartite_greedy

OPTS = list(ec.OPTION_SETS)


def enc_of(opt):
    return ec.small_encoder(**ec.OPTION_SETS[opt])


def state(enc, row):
    """'positive' | 'neutral' | 'background' of one encoded row."""
    cls = row[:enc.n_classes]
    if cls.sum() == 0:
        return "neutral"
    return "background" if cls[enc.background_id] == 1 else "positive"      # the cases here use no background-class box


def test_small_family_and_option_axes():
    seen = {k: set() for k in ("border_pixels", "normalize_coords", "clip_boxes", "background_id", "matching_type",
                               "neutral_possible", "variances", "steps")}
    base = enc_of("default").generate_encoding_template(1)[0]
    for opt in OPTS:
        kw = ec.small_kwargs(**ec.OPTION_SETS[opt])
        enc = ec.small_encoder(**ec.OPTION_SETS[opt])
        t = enc.generate_encoding_template(1)[0]
        assert t.shape == (ec.SMALL_ANCHORS, ec.SMALL_CLASSES + 1 + 12) and ec.SMALL_ANCHORS % 64 == 4
        for k in ("border_pixels", "normalize_coords", "clip_boxes", "matching_type"):
            seen[k].add(kw[k])
        seen["background_id"].add(kw["background_id"] != 0)
        seen["neutral_possible"].add(kw["matching_type"] == "bipartite" or kw["neg_iou_limit"] < kw["pos_iou_threshold"])
        seen["variances"].add(tuple(kw["variances"]) != (0.1, 0.1, 0.2, 0.2))
        seen["steps"].add(kw["steps"] is not None)
        if kw["border_pixels"] != "half":          # the log of a negative normalised width is not finite on the host
            assert not kw["normalize_coords"]
        if kw["clip_boxes"]:                        # clipping moves anchors of this family
            plain = ec.small_encoder(**dict(ec.OPTION_SETS[opt], clip_boxes=False)).generate_encoding_template(1)[0]
            assert (plain[:, -8:-4] != t[:, -8:-4]).any()
        if kw["steps"] is not None:
            assert (base[:, -8:-6] != t[:, -8:-6]).any() or not kw["normalize_coords"]
    assert seen["border_pixels"] == {"half", "include", "exclude"}
    assert all(v == {False, True} for k, v in seen.items() if k not in ("border_pixels", "matching_type"))
    assert seen["matching_type"] == {"multi", "bipartite"}
    assert any(ec.OPTION_SETS[o].get("background_id", 0) == ec.SMALL_CLASSES for o in OPTS)    # the last column


@pytest.mark.parametrize("opt", OPTS)
def test_every_case_is_finite_and_well_formed(opt):
    enc = enc_of(opt)
    images, spans = ec.batch(enc)
    assert [s[0] for s in spans] == list(ec.CASES) and spans[-1][2] == len(images)
    y = enc(images)
    assert np.isfinite(y).all()
    for g in images:
        assert g.shape[1:] == (5,) and g.dtype == np.float64
        if len(g):
            sim = ec.similarities(enc, g)
            assert np.isfinite(sim).all() and sim.min() >= 0       # zeroed entries and true zeros are the row minimum
            assert (g[:, 0] >= 0).all() and (g[:, 0] < enc.n_classes).all()
    counts = [len(g) for g in images]
    assert counts[0] == 0 and max(counts) == 128 and sorted(counts)[len(counts) // 2] <= 4     # mostly padding rows
    hi = enc.n_classes - 1
    ids = np.concatenate([g[:, 0] for g in ec.CASES["class_ids"](enc)])
    assert {0, hi} <= set(ids.tolist())
    sweep = ec.sweep(enc, seed=1, n_images=60)
    assert np.isfinite(enc(sweep)).all()
    sims = [ec.similarities(enc, g) for g in sweep if len(g)]
    assert min(s.min() for s in sims) >= 0 and sum((s.max(1) == 0).sum() for s in sims) >= 10     # boxes outside everything
    assert {len(g) for g in sweep} >= {0, 12}


@pytest.mark.parametrize("opt", OPTS)
def test_quirk_cases_orphan_an_anchor(opt):
    enc = enc_of(opt)
    multi = enc.matching_type == "multi"
    want = "positive" if multi else "neutral"
    for name, orphans, kept in [("quirk_matched_then_far", [ec.ORPHAN], []), ("quirk_two_far", [ec.ORPHAN], [50]),
                                ("quirk_orphan_neutral", [ec.ORPHAN], [60])]:
        (g,) = ec.CASES[name](enc)
        sim = ec.similarities(enc, g)
        first = match_bipartite_greedy(sim)
        assert first[0] == 0 and (first == 0).sum() >= 2, (name, first)             # the duplicated anchor 0
        y = enc([g])[0]
        for a in orphans:
            assert sim[0].argmax() == a and a not in first
            assert sim[0, a] >= max(enc.pos_iou_threshold, enc.neg_iou_limit)
            assert state(enc, y[a]) == want, (name, a)
            if multi:
                assert y[a, int(g[0, 0])] == 1
        for a in kept:
            assert a in first and state(enc, y[a]) == "positive"
        last = int(np.nonzero(first == 0)[0][-1])                                    # anchor 0: the last ground truth wins
        assert y[0, int(g[last, 0])] == 1 and np.isfinite(y[0]).all() and state(enc, y[0]) == "positive"
    # the zero-overlap box first: nothing is orphaned, the far box sits on anchor 0
    (g,) = ec.CASES["quirk_far_then_matched"](enc)
    sim = ec.similarities(enc, g)
    assert (sim[0] == 0).all() and match_bipartite_greedy(sim).tolist() == [0, ec.ORPHAN]
    (g,) = ec.CASES["quirk_all_far"](enc)
    sim = ec.similarities(enc, g)
    assert (sim == 0).all() and match_bipartite_greedy(sim).tolist() == [0, 0, 0]
    y = enc([g])[0]
    assert y[0, int(g[-1, 0])] == 1 and [state(enc, r) for r in y[1:]] == ["background"] * (ec.SMALL_ANCHORS - 1)


def test_quirk_ssd300_case_is_the_reported_one():
    enc = ec.encoder(ec.SIZES["custom"])
    (g,) = ec.SSD300_CASES["quirk_matched_then_far"](enc)
    sim = ec.similarities(enc, g)
    first = match_bipartite_greedy(sim)
    assert first.tolist() == [0, 0] and (sim[1] == 0).all()
    y = enc([g])[0]
    assert (y[:, 1:21].sum(-1) > 0).sum() == 17 and y[sim[0].argmax(), 3] == 1


@pytest.mark.parametrize("opt", OPTS)
def test_identical_boxes_share_their_first_choice(opt):
    enc = enc_of(opt)
    for n in (5, 20):
        (g,) = ec.CASES["identical_%d" % n](enc)
        sim = ec.similarities(enc, g)
        assert len(g) == n and len(set(sim.argmax(1).tolist())) == 1 and (sim == sim[0]).all()
        first = match_bipartite_greedy(sim)
        assert len(set(first.tolist())) == n and sim[0, first].min() > 0       # n - 1 rows redone after the first match
        assert len(set(g[:, 0].tolist())) == enc.n_classes
    assert 20 - 1 > 16                                                           # a redo list longer than the 16 waves
    (g,) = ec.CASES["tie_two_identical"](enc)
    sim = ec.similarities(enc, g)
    assert (sim[0] == sim[1]).all() and g[0, 0] != g[1, 0]
    first = match_bipartite_greedy(sim)
    met = np.nonzero((sim[0] >= enc.pos_iou_threshold) & ~np.isin(np.arange(sim.shape[1]), first))[0]
    if enc.matching_type == "multi":
        y = enc([g])[0]
        assert len(met) >= 1 and all(y[a, int(g[0, 0])] == 1 and y[a, int(g[1, 0])] == 0 for a in met)   # lowest gt wins


@pytest.mark.parametrize("opt", OPTS)
def test_index_edge_cases_match_the_named_anchors(opt):
    enc = enc_of(opt)
    images = ec.CASES["index_edges"](enc)
    want = [0, ec.SMALL_ANCHORS - 1, 63, 64]
    assert match_bipartite_greedy(ec.similarities(enc, images[0])).tolist() == want
    assert ec.similarities(enc, images[0]).argmax(1).tolist() == want
    for g, a in zip(images[1:], want):
        assert ec.similarities(enc, g).argmax(1).tolist() == [a]


def test_index_edge_case_ssd300():
    enc = ec.encoder(ec.SIZES["custom"])
    images = ec.SSD300_CASES["index_edges_1023_1024"](enc)
    assert ec.similarities(enc, images[0]).argmax(1).tolist() == [0, 8731, 1023, 1024]
    (g,) = ec.SSD300_CASES["cap_128"](enc)
    first = match_bipartite_greedy(ec.similarities(enc, g))
    assert len(g) == 128 and len(set(first.tolist())) == 128 and len(np.unique(g[:, 1:], axis=0)) == 128


@pytest.mark.parametrize("opt", OPTS)
def test_tie_cases_have_bit_equal_overlaps(opt):
    enc = enc_of(opt)
    kw = ec.small_kwargs(**ec.OPTION_SETS[opt])
    (g,) = ec.CASES["tie_between_anchors"](enc)
    sim = ec.similarities(enc, g)[0]
    assert sim[0] == sim[4] > 0                           # the two anchors it lies between: bit-equal
    if kw["border_pixels"] == "half" and kw["steps"] is None:
        at_max = np.nonzero(sim == sim.max())[0]          # and the row maximum is shared by two mirror-image anchors
        assert len(at_max) == 2 and match_bipartite_greedy(sim[None])[0] == at_max[0]
    enc2, images, a = ec.twin_case(**ec.OPTION_SETS[opt])
    t = enc2.generate_encoding_template(1)[0]
    assert t.shape[0] == 85 and (t[a] == t[a + 1]).all()
    for g in images:
        sim = ec.similarities(enc2, g)
        assert sim[0, a] == sim[0, a + 1] == sim[0].max() and match_bipartite_greedy(sim)[0] == a
        y = enc2([g])[0]
        assert state(enc2, y[a]) == "positive"
        assert state(enc2, y[a + 1]) == ("positive" if enc2.matching_type == "multi" else "neutral")


@pytest.mark.parametrize("opt", OPTS)
def test_threshold_cases_sit_on_the_threshold(opt):
    o = ec.OPTION_SETS[opt]
    for which in ("pos", "neg"):
        enc, images, a, kw = ec.threshold_case(which, **o)
        sim = ec.similarities(enc, images[0])
        first = match_bipartite_greedy(sim)
        thr = enc.pos_iou_threshold if which == "pos" else enc.neg_iou_limit
        assert a not in first and sim[0, a] == thr                     # bit-equal: `>=` against `>` decides row a
        y = enc(images)[0]
        assert np.isfinite(y).all()
        above = np.nextafter(thr, 2.0)                                  # one ulp higher and the row is background
        if which == "pos":
            assert state(enc, y[a]) == "positive"
            other = ec.small_encoder(**dict(kw, pos_iou_threshold=above, neg_iou_limit=above))
        else:
            assert state(enc, y[a]) == "neutral"
            other = ec.small_encoder(**dict(kw, neg_iou_limit=above))
        assert state(enc, other(images)[0][a]) == "background"


def test_caps_are_the_kernels():
    enc = enc_of("default")
    (g,) = ec.CASES["cap_128"](enc)
    assert len(g) == 128 > ec.SMALL_ANCHORS                 # more boxes than anchors: the late rounds are all empty
    first = match_bipartite_greedy(ec.similarities(enc, g))
    assert (first == 0).sum() > 128 - ec.SMALL_ANCHORS
    big = ec.small_encoder(predictor_sizes=[(56, 56), (2, 2), (1, 1)])
    assert big.generate_encoding_template(1).shape[1] == 56 * 56 * 4 + 20 > 12288
