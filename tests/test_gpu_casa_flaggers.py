"""-m gpu: the CASA-style baseline flaggers (csrc/casa_flaggers.hip) against the NumPy oracle tests/casa_flaggers_ref.py.
Every comparison is bit equality of the flags: the header pins the order of every operation, the library is built without
contraction, so a differing flag is a differing operation.  (The pipelines expose no float stage; every float decides a
flag through a strict comparison, and the planes below carry features faint enough to sit near those comparisons.)"""
import numpy as np
import pytest

import casa_flaggers_ref as ref
from oracle import synth_ref
from test_sumthreshold_host import EVENTS

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def fl():
    from rfi_toolbox_amd import flagging
    return flagging


def _same(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == bool and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def _noisy(rng, shape, spikes=3):
    """complex128 around a sloping level with a few bright samples and one step."""
    C, T = shape
    amp = (1.0 + 0.3 * np.arange(C)[:, None] / max(C, 1)) * (1.0 + 0.1 * rng.standard_normal(shape))
    for _ in range(spikes):
        amp[rng.integers(C), rng.integers(T)] += 3.0
    amp[C // 2, T // 3:] += 0.4
    z = amp * np.exp(0.3j * rng.standard_normal(shape))
    return z


# ---------------------------------------------------------------------------------------------- line lengths
@pytest.mark.parametrize("axis", [-1, -2])
@pytest.mark.parametrize("L", LENGTHS)
def test_line_lengths(fl, axis, L):
    rng = np.random.default_rng(200 + L)
    shape = (5, L) if axis == -1 else (L, 5)
    z = _noisy(rng, shape)
    prior = rng.random(shape) < 0.1
    x = np.abs(z).astype(np.float32)
    for shape_name in ("line", "poly"):
        for pieces in (1, 3, 7):
            kw = dict(timefit=shape_name, freqfit=shape_name, maxnpieces=pieces, timecutoff=2.5, freqcutoff=2.5)
            _same(fl.tfcrop_flags(x, flags=prior, **kw), ref.tfcrop(x, prior, **kw), (shape_name, pieces))
    for winsize in (1, 3, 7):
        kw = dict(winsize=winsize, timedevscale=1.5, freqdevscale=1.5)
        _same(fl.rflag_flags(z, flags=prior, **kw), ref.rflag(z, prior, **kw), winsize)
    kw = dict(growaround=True, flagneartime=True, flagnearfreq=True, growtime=60.0, growfreq=60.0)
    _same(fl.extend_flags(prior, **kw), ref.extend(prior, **kw))


# ---------------------------------------------------------------------------------------------- tile boundaries
@pytest.mark.parametrize("shape", [(33, 1100), (1100, 33)])
def test_across_tile_boundaries(fl, shape):
    """The builder's tiles: the transposes move 32 x 32 tiles; the fit gives a workgroup 64 adjacent lines (channels for
    the time stage, time samples for the frequency stage); the selection and growtime kernels stride a line by 64; the
    elementwise kernels take 256 samples per workgroup.  A faint run is laid across every multiple of 32 along the long
    axis, on the lines 0, 31 and 32 of the short one, and the chunks (700 time samples of 1100, 20 of 33) end on no
    multiple of any of them."""
    rng = np.random.default_rng(shape[0])
    C, T = shape
    amp = 1.0 + 0.05 * rng.standard_normal(shape)
    long_axis = 1 if T > C else 0
    for b in range(32, max(C, T) - 4, 32):
        for other in (0, 31, 32):
            if long_axis == 1:
                amp[other % C, b - 3:b + 3] += 0.16 + 0.02 * (b // 32 % 5)
            else:
                amp[b - 3:b + 3, other % T] += 0.16 + 0.02 * (b // 32 % 5)
    z = amp * np.exp(0.2j * rng.standard_normal(shape))
    prior = rng.random(shape) < 0.02
    ntime = 700 if long_axis == 1 else 20
    want = ref.tfcrop(z, prior, ntime=ntime)
    _same(fl.tfcrop_flags(z, flags=prior, ntime=ntime), want)
    assert (want & ~prior).any() and not want.all()
    kw = dict(ntime=ntime, timedevscale=2.5, freqdevscale=2.5)
    want = ref.rflag(z, prior, **kw)
    _same(fl.rflag_flags(z, flags=prior, **kw), want)
    assert (want & ~prior).any() and not want.all()
    dense = rng.random(shape) < 0.45
    kw = dict(ntime=ntime, growaround=True, flagneartime=True, flagnearfreq=True, growtime=47.0, growfreq=47.0)
    _same(fl.extend_flags(dense, **kw), ref.extend(dense, **kw))


# ---------------------------------------------------------------------------------------------- chunking
@pytest.mark.parametrize("ntime", [1, 32, 69, 70, 500, None])
def test_ntime_chunks(fl, ntime):
    rng = np.random.default_rng(70)
    z = _noisy(rng, (24, 70), spikes=8)
    prior = rng.random(z.shape) < 0.05
    if ntime == 1:                           # (one-sample chunks: many tiny fits for the oracle, so a smaller plane)
        z, prior = z[:8, :10].copy(), prior[:8, :10].copy()
    _same(fl.tfcrop_flags(z, flags=prior, ntime=ntime), ref.tfcrop(z, prior, ntime=ntime))
    for dim in ("timefreq", "time", "freq"):
        _same(fl.tfcrop_flags(z, ntime=ntime, flagdimension=dim, timefit="poly", maxnpieces=4),
              ref.tfcrop(z, ntime=ntime, flagdimension=dim, timefit="poly", maxnpieces=4), dim)
    kw = dict(ntime=ntime, timedevscale=2.0, freqdevscale=2.0)
    _same(fl.rflag_flags(z, flags=prior, **kw), ref.rflag(z, prior, **kw))
    kw = dict(ntime=ntime, growaround=True, flagneartime=True, growtime=20.0)
    _same(fl.extend_flags(prior, **kw), ref.extend(prior, **kw))


# ---------------------------------------------------------------------------------------------- flagged lines, bad values
def test_flagged_lines_and_non_finite_values(fl):
    rng = np.random.default_rng(5)
    z = np.stack([_noisy(rng, (20, 40)) for _ in range(4)])
    prior = np.zeros(z.shape, bool)
    prior[0, 7, :] = True                    # a channel
    prior[1, :, 11] = True                   # a time sample
    prior[2] = True                          # a plane
    z[3, 4, 5] = complex(np.nan, 1.0)
    z[3, 9, 30] = complex(1.0, np.inf)
    z[3, 10, 0] = complex(-np.inf, np.nan)
    for got, want in ((fl.tfcrop_flags(z, flags=prior), ref.tfcrop(z, prior)),
                      (fl.rflag_flags(z, flags=prior, timedevscale=2.0, freqdevscale=2.0),
                       ref.rflag(z, prior, timedevscale=2.0, freqdevscale=2.0))):
        _same(got, want)
        assert (got | ~prior).all() and got[2].all() and got[3, 4, 5] and got[3, 9, 30] and got[3, 10, 0]
        assert not got[0].all() and not got[3].all()
    # float64 magnitudes that overflow float32 are flagged, a constant plane gets no flag
    x = np.abs(z[0])
    x[3, 3] = 1e300
    want = ref.tfcrop(x)
    _same(fl.tfcrop_flags(x), want)
    assert want[3, 3]
    const = np.full((6, 9), 0.75 + 0.25j)
    assert not fl.tfcrop_flags(const).any() and not fl.rflag_flags(const).any()
    assert fl.tfcrop_flags(np.array([[np.inf]], np.float32)).tolist() == [[True]]
    assert fl.rflag_flags(np.array([[3.0 + 4.0j]])).tolist() == [[False]]


# ---------------------------------------------------------------------------------------------- a stack of planes
def test_stack_of_planes_keeps_its_planes_apart(fl):
    rng = np.random.default_rng(9)
    base = _noisy(rng, (30, 50), spikes=6)
    noise = rng.standard_normal((3, 30, 50)) + 1j * rng.standard_normal((3, 30, 50))
    z = np.stack([base * lvl + 0.05 * lvl * s * noise[i] for i, (lvl, s) in enumerate(((1.0, 1.0), (40.0, 2.0), (0.01, 4.0)))])
    z = z.reshape(3, 1, 30, 50)
    kw = dict(timedevscale=2.5, freqdevscale=2.5)
    for got, want in ((fl.tfcrop_flags(z), ref.tfcrop(z)), (fl.rflag_flags(z, **kw), ref.rflag(z, **kw))):
        _same(got, want)
        assert len({want[i].tobytes() for i in range(3)}) == 3 and all(want[i].any() for i in range(3))
    # thresholds given per plane and per (plane, channel)
    td, fd = np.array([0.1, 4.0, 0.001]), np.array([0.2, 8.0, 0.002])
    _same(fl.rflag_flags(z, timedev=td, freqdev=fd), ref.rflag(z, timedev=td, freqdev=fd))
    tdc = td[:, None] * (1.0 + 0.5 * rng.random((3, 30)))
    _same(fl.rflag_flags(z, timedev=tdc.reshape(3, 1, 30), freqdev=0.3), ref.rflag(z, timedev=tdc, freqdev=0.3))
    _same(fl.rflag_flags(z, timedev=0.1), ref.rflag(z, timedev=0.1))


# ---------------------------------------------------------------------------------------------- dtypes and input forms
def test_dtypes_and_input_forms(fl):
    import torch
    from rfi_toolbox_amd.runtime import Context
    ctx = Context.get(0)
    rng = np.random.default_rng(21)
    z128 = np.stack([_noisy(rng, (17, 33)) for _ in range(2)])
    prior = rng.random(z128.shape) < 0.05
    z64 = z128.astype(np.complex64)
    low = dict(timedevscale=2.0, freqdevscale=2.0)
    for z in (z128, z64):
        want_t, want_r = ref.tfcrop(z, prior), ref.rflag(z, prior, **low)
        assert (want_t | ~prior).all() and (want_r | ~prior).all() and (want_t & ~prior).any() and (want_r & ~prior).any()
        _same(fl.tfcrop_flags(z, flags=prior), want_t)
        _same(fl.rflag_flags(z, flags=prior, **low), want_r)
        _same(fl.tfcrop_flags(z, flags=prior.view(np.uint8) * 5), want_t)
        # torch on the host, torch on the device, DeviceArray
        _same(fl.tfcrop_flags(torch.from_numpy(z), flags=torch.from_numpy(prior)), want_t)
        _same(fl.rflag_flags(torch.from_numpy(z), flags=torch.from_numpy(prior), **low), want_r)
        got = fl.tfcrop_flags(torch.from_numpy(z).cuda(), flags=torch.from_numpy(prior).cuda())
        assert got.is_cuda and got.dtype == torch.bool
        _same(got.cpu().numpy(), want_t)
        got = fl.rflag_flags(torch.from_numpy(z).cuda(), flags=torch.from_numpy(prior).cuda(), **low)
        assert got.is_cuda and got.dtype == torch.bool
        _same(got.cpu().numpy(), want_r)
        dz, dp = ctx.to_device(z), ctx.to_device(prior.view(np.uint8))
        for got, want in ((fl.tfcrop_flags(dz, flags=dp, out="device"), want_t), (fl.rflag_flags(dz, flags=dp, out="device", **low), want_r)):
            assert got.dtype == np.uint8 and got.shape == z.shape
            assert got.numpy().tobytes() == want.view(np.uint8).tobytes()
        _same(fl.tfcrop_flags(dz, flags=dp), want_t)
    for x in (np.abs(z128), np.abs(z128).astype(np.float32)):
        _same(fl.tfcrop_flags(x, flags=prior), ref.tfcrop(x, prior))
    # extend: the same forms
    kw = dict(growaround=True, flagneartime=True, growtime=30.0)
    want = ref.extend(prior, **kw)
    _same(fl.extend_flags(prior, **kw), want)
    _same(fl.extend_flags(prior.view(np.uint8) * 9, **kw), want)
    _same(fl.extend_flags(torch.from_numpy(prior), **kw), want)
    got = fl.extend_flags(torch.from_numpy(prior).cuda(), **kw)
    assert got.is_cuda and got.dtype == torch.bool
    _same(got.cpu().numpy(), want)
    got = fl.extend_flags(ctx.to_device(prior.view(np.uint8)), out="device", **kw)
    assert got.dtype == np.uint8 and got.numpy().tobytes() == want.view(np.uint8).tobytes()


# ---------------------------------------------------------------------------------------------- extend
EXTEND_OPTIONS = [dict(growtime=100.0, growfreq=100.0), dict(growtime=100.0, growfreq=100.0, growaround=True),
                  dict(growtime=30.0, growfreq=100.0), dict(growtime=100.0, growfreq=30.0), dict(growtime=0.0, growfreq=100.0),
                  dict(growtime=100.0, growfreq=100.0, flagneartime=True), dict(growtime=100.0, growfreq=100.0, flagnearfreq=True),
                  dict(), dict(growtime=35.0, growfreq=45.0, growaround=True, flagneartime=True, flagnearfreq=True)]


@pytest.mark.parametrize("shape", [(40, 70), (1, 7), (5, 1)])
def test_extend_every_option(fl, shape):
    rng = np.random.default_rng(shape[1])
    masks = np.stack([rng.random(shape) < d for d in (0.0, 0.1, 0.35, 0.5, 0.9, 1.0)])
    changed = 0
    for kw in EXTEND_OPTIONS:
        for ntime in (None, 32):
            want = ref.extend(masks, ntime=ntime, **kw)
            _same(fl.extend_flags(masks, ntime=ntime, **kw), want, (kw, ntime))
            assert (want | ~masks).all()
            changed += int((want != masks).any())
    assert changed >= (10 if shape == (40, 70) else 2)
    # exactly half a line is not grown, one more sample is
    half = np.zeros((4, 8), bool)
    half[1, :4] = True
    half[2, :5] = True
    got = fl.extend_flags(half, growfreq=100.0)
    assert np.array_equal(got[1], half[1]) and got[2].all() and not got[0].any()


# ---------------------------------------------------------------------------------------------- the whole pipelines
@pytest.fixture(scope="module")
def synthetic():
    planes, _ = synth_ref.generate(7, EVENTS, 2, 96, 160, noise=0.1, use_bandpass=False)
    return planes, ref.tfcrop(planes), ref.rflag(planes)


def test_pipelines_on_the_synthetic_planes(fl, synthetic):
    planes, want_t, want_r = synthetic
    _same(fl.tfcrop_flags(planes), want_t)
    _same(fl.rflag_flags(planes), want_r)
    assert want_t[:2].any() and want_r[:2].any() and not want_t.all()
    dev = fl.tfcrop_flags(planes, out="device")
    kw = dict(growaround=True, flagneartime=True, flagnearfreq=True, growtime=40.0, growfreq=40.0)
    want = ref.extend(want_t, **kw)
    _same(fl.extend_flags(dev, out="host", **kw), want)
    assert (want != want_t).any()
    _same(fl.extend_flags(fl.rflag_flags(planes, out="device"), ntime=64, **kw), ref.extend(want_r, ntime=64, **kw))


def test_stage_planes(fl):
    """The planes of the host test on which dropping any stage changes the answer."""
    from test_casa_flaggers_host import rflag_plane, stage_plane
    z = stage_plane()
    _same(fl.tfcrop_flags(z), ref.tfcrop(z))
    for kw in (dict(flagdimension="time"), dict(maxnpieces=1), dict(flagdimension="timefreq"), dict(ntime=32)):
        _same(fl.tfcrop_flags(z, **kw), ref.tfcrop(z, **kw), kw)
    z = rflag_plane()
    for kw in (dict(), dict(freqdev=1e30), dict(timedev=1e30), dict(winsize=5)):
        _same(fl.rflag_flags(z, **kw), ref.rflag(z, **kw), kw)


def test_reproducibility(fl, synthetic):
    planes, want_t, want_r = synthetic
    c64 = planes.astype(np.complex64)
    a, b = fl.tfcrop_flags(c64), fl.tfcrop_flags(c64)
    assert a.tobytes() == b.tobytes()
    a, b = fl.rflag_flags(c64, ntime=50), fl.rflag_flags(c64, ntime=50)
    assert a.tobytes() == b.tobytes()
    a, b = fl.extend_flags(want_t, growaround=True), fl.extend_flags(want_t, growaround=True)
    assert a.tobytes() == b.tobytes()
