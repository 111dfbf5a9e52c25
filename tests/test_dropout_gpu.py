"""dj_dropout_fwd / dj_dropout_bwd against the host statement (keras/dropout.py), bit for bit: sizes around the group of
four and the tail, a size that takes the grid-stride loop round more than once, the three rates, a base pointer that is
not 16-byte aligned, in place, beta 0 / 1, Inf and NaN on kept and dropped positions, and the argument checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TRIPLES = [(17, 0, 3), (0xC0FFEE11, 5, 2 ** 32 + 9)]      # (seed, rank, step); the second carries a step above 32 bits


def _lib():
    from jpeg_detection_resnet_ssd_amd import _lib
    return _lib.load()


def _several_passes():
    """Smallest interesting n for which threads of the capped grid take a second group: the cap is the launcher's."""
    return 4 * int(_lib().dj_dropout_groups_per_pass()) + 4 * 1000 + 3


def _same_bits(got, want):
    """Equal bit for bit, NaNs at the same positions (their payloads are not compared)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _words(rate, triple):
    from jpeg_detection_resnet_ssd_amd.keras import dropout as D
    return (D.dropout_threshold(rate), float(D.dropout_scale(rate))) + D.dropout_words(*triple)


def _fwd(x, y, n, rate, triple):
    from jpeg_detection_resnet_ssd_amd.engine import call
    call("dj_dropout_fwd", x, y, n, *_words(rate, triple))


def _bwd(dy, dx, n, rate, triple, beta):
    from jpeg_detection_resnet_ssd_amd.engine import call
    call("dj_dropout_bwd", dy, dx, n, *(_words(rate, triple) + (beta,)))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(77)
    n = _several_passes()
    return rng.standard_normal(n + 1).astype(np.float32), rng.standard_normal(n + 1).astype(np.float32)


@pytest.mark.parametrize("rate", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 8192, "several passes"])
def test_forward_and_backward_equal_the_host_statement(cuda, data, n, rate):
    from jpeg_detection_resnet_ssd_amd.keras.dropout import dropout_host
    n = _several_passes() if n == "several passes" else n
    xs, ds = data
    triples = TRIPLES if n <= 8192 else TRIPLES[:1]
    for triple in triples:
        for off in (0, 1):        # off 1: a [1:] view of an aligned buffer, so the 16-byte path must fall back
            xh, dh = xs[off:off + n], ds[off:off + n]
            want = dropout_host(xh, rate, *triple)
            xbuf = torch.from_numpy(xs[:n + 1].copy()).to(cuda)
            x = xbuf[off:off + n]
            assert (x.data_ptr() % 16 == 0) == (off == 0)
            y = torch.full((n + 2,), 7.0, device=cuda)[off:off + n + 1]
            _fwd(x, y, n, rate, triple)
            yh = y.cpu().numpy()
            _same_bits(yh[:n], want)
            assert yh[n] == 7.0                                  # nothing past the end
            assert np.array_equal(x.cpu().numpy(), xh)           # the input is left alone
            _fwd(x, x, n, rate, triple)                          # in place
            _same_bits(x.cpu().numpy(), want)
            grad = dropout_host(dh, rate, *triple)
            dy = torch.from_numpy(ds[:n + 1].copy()).to(cuda)[off:off + n]
            for beta in (0, 1):
                dx = torch.from_numpy(xs[:n + 1].copy()).to(cuda)[off:off + n]
                _bwd(dy, dx, n, rate, triple, beta)
                _same_bits(dx.cpu().numpy(), xh + grad if beta else grad)
    if n >= 8:
        a, b = (dropout_host(xs[:n], rate, *t) for t in TRIPLES)
        assert not np.array_equal(a == 0, b == 0)                # the two triples draw different masks


def test_inf_and_nan_on_kept_and_dropped_positions(cuda):
    from jpeg_detection_resnet_ssd_amd.keras.dropout import dropout_host, dropout_keep_host
    n, rate, triple = 1021, 0.5, TRIPLES[0]
    keep = dropout_keep_host(n, rate, *triple)
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    xh = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    xh[kept[0]], xh[dropped[0]] = np.inf, np.inf
    xh[kept[1]], xh[dropped[1]] = np.nan, np.nan
    xh[kept[2]], xh[dropped[2]] = -np.inf, -np.inf
    want = dropout_host(xh, rate, *triple)
    assert np.isinf(want[kept[0]]) and np.isnan(want[dropped[0]]) and np.isnan(want[kept[1]]) and np.isnan(want[dropped[2]])
    x = torch.from_numpy(xh).to(cuda)
    y = torch.empty_like(x)
    _fwd(x, y, n, rate, triple)
    _same_bits(y.cpu().numpy(), want)
    for beta in (0, 1):
        dx = torch.ones(n, device=cuda)
        _bwd(x, dx, n, rate, triple, beta)
        _same_bits(dx.cpu().numpy(), np.float32(1.0) + want if beta else want)


def test_bad_arguments_are_refused_before_any_launch(cuda):
    lib = _lib()
    x = torch.ones(8, device=cuda)
    p = x.data_ptr()
    w = (2 ** 31, 2.0, 1, 0, 0, 0)
    assert lib.dj_dropout_fwd(None, p, 8, *w, None) == -1
    assert b"dj_dropout_fwd" in lib.dj_last_error()
    assert lib.dj_dropout_fwd(p, None, 8, *w, None) == -1
    assert lib.dj_dropout_fwd(p, p, 0, *w, None) == -1
    assert lib.dj_dropout_fwd(p, p, -4, *w, None) == -1
    assert lib.dj_dropout_bwd(None, p, 8, *w, 0, None) == -1
    assert b"dj_dropout_bwd" in lib.dj_last_error()
    assert lib.dj_dropout_bwd(p, None, 8, *w, 0, None) == -1
    assert lib.dj_dropout_bwd(p, p, 0, *w, 1, None) == -1
    assert lib.dj_dropout_bwd(p, p, 8, *w, 2, None) == -1
    torch.cuda.synchronize()
    assert bool((x == 1).all())
