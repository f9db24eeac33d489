"""-m gpu: the SumThreshold baseline flagger (csrc/sumthreshold.hip) against the NumPy oracle tests/sumthreshold_ref.py.
Every comparison is bit equality: the header pins the order of every operation, the library is built without
contraction, so a differing bit is a differing operation."""
import numpy as np
import pytest

import sumthreshold_ref as ref
from oracle import synth_ref

pytestmark = pytest.mark.gpu

EVENTS = [[(0, 20, 21, 0, 160, 5.0), (0, 0, 96, 40, 42, 3.0), (0, 60, 61, 30, 94, 0.15), (1, 10, 80, 4, 1, 2.0)],
          [(0, 5, 7, 0, 160, 1.0), (0, 50, 51, 100, 108, 0.8)],
          []]
CONFIGS = {"defaults": {}, "short": dict(iterations=2, levels=4, rho=1.3, sir_eta=0.0)}
WINDOWS = (1, 2, 8, 64, 128)


@pytest.fixture(scope="module")
def fl():
    from rfi_toolbox_amd import flagging
    return flagging


def _ref_pass(v, f, M, th, ce, axis):
    v, f = v.reshape((-1,) + v.shape[-2:]), f.reshape((-1,) + f.shape[-2:])
    th, ce = np.broadcast_to(np.asarray(th, np.float64).reshape(-1), len(v)), np.broadcast_to(np.asarray(ce, np.float64).reshape(-1), len(v))
    return np.stack([ref.sumthreshold_pass(v[i], f[i], M, th[i], ce[i], axis=axis) for i in range(len(v))])


# ---------------------------------------------------------------------------------------------- sumthreshold_pass
@pytest.mark.parametrize("axis", [-1, -2])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])
def test_pass_line_lengths_and_windows(fl, axis, L):
    rng = np.random.default_rng(100 + L)
    shape = (5, L) if axis == -1 else (L, 5)
    v = rng.standard_normal(shape).astype(np.float32)
    f = rng.random(shape) < 0.1
    for M in WINDOWS:
        th = 2.0 / np.sqrt(M)                      # a few per cent of the windows hit
        want = ref.sumthreshold_pass(v, f, M, th, 0.25, axis=axis)
        got = fl.sumthreshold_pass(v, f, M, th, center=0.25, axis=axis)
        assert got.dtype == bool and np.array_equal(got, want), (M, int((got != want).sum()))
        if M <= L:
            assert (want & ~f).any() or L < 8
        else:
            assert np.array_equal(got, f)


def test_pass_stack_with_per_plane_center_and_threshold(fl):
    rng = np.random.default_rng(7)
    v = (rng.standard_normal((3, 40, 70)) + np.array([0.0, 2.0, -1.0])[:, None, None]).astype(np.float32)
    f = rng.random(v.shape) < 0.05
    th, ce = np.array([1.0, 0.6, 3.0]), np.array([0.0, 2.0, -1.0])
    for axis in (-1, -2):
        for M in (1, 4, 32):
            want = _ref_pass(v, f, M, th, ce, axis)
            got = fl.sumthreshold_pass(v, f, M, th, center=ce, axis=axis)
            assert np.array_equal(got, want), (axis, M)
    assert len({int(w.sum()) for w in _ref_pass(v, f, 1, th, ce, -1)}) == 3


@pytest.mark.parametrize("shape", [(33, 1100), (1100, 33)])
def test_pass_across_tile_boundaries(fl, shape):
    """The time kernel gives a workgroup 641 - M window starts of one row; the frequency kernel 161 - M window starts of
    32 adjacent time samples.  A faint run that only its own window catches is laid across each boundary of both."""
    rng = np.random.default_rng(shape[0])
    C, T = shape
    for M in (1, 8, 128):
        for axis, L, step in ((-1, T, 641 - M), (-2, C, 161 - M)):
            if M > L:
                continue
            v = (0.1 * rng.standard_normal(shape)).astype(np.float32)
            for b in range(step, L - M // 2, step):             # a run of M samples centred on every tile boundary
                lo = max(0, b - M // 2)
                for other in (0, 31, 32):                        # rows / columns on both sides of the 32-column boundary
                    if axis == -1:
                        v[other % C, lo:lo + M] += 1.0
                    else:
                        v[lo:lo + M, other % T] += 1.0
            f = rng.random(shape) < 0.02
            th = 0.7 if M > 1 else 0.9
            want = ref.sumthreshold_pass(v, f, M, th, 0.0, axis=axis)
            got = fl.sumthreshold_pass(v, f, M, th, axis=axis)
            assert np.array_equal(got, want), (M, axis, int((got != want).sum()))
            assert (want & ~f).any() or L <= step


def test_pass_all_flagged_line(fl):
    v = np.full((4, 200), 50.0, np.float32)
    f = np.zeros((4, 200), bool)
    f[1] = True
    f[:, 100] = True
    for axis in (-1, -2):
        for M in (1, 4):
            got = fl.sumthreshold_pass(v, f, M, 1e9, axis=axis)
            assert np.array_equal(got, f)
            got = fl.sumthreshold_pass(v, f, M, 1.0, axis=axis)
            assert np.array_equal(got, ref.sumthreshold_pass(v, f, M, 1.0, axis=axis)) and got.all()
    assert np.array_equal(fl.sumthreshold_pass(v, np.ones_like(f), 2, 0.0), np.ones_like(f))


# ---------------------------------------------------------------------------------------------- masked_gaussian_smooth
@pytest.mark.parametrize("shape", [(17, 33), (1, 7), (5, 1), (70, 300)])
def test_smooth_bit_equal(fl, shape):
    rng = np.random.default_rng(shape[1])
    v = (3.0 + rng.standard_normal(shape) * np.linspace(0.5, 2.0, shape[1])).astype(np.float32)
    f = rng.random(shape) < 0.3
    if shape == (70, 300):
        f[10:60, 100:200] = True               # wider than the window in both directions: D2 == 0 inside
    wt, wf = fl.gaussian_weights(2.5, 10), fl.gaussian_weights(5.0, 15)     # half widths past the small planes' edges
    want = ref.masked_gaussian_smooth(v, f, wt, wf)
    got = fl.masked_gaussian_smooth(v, f, wt, wf)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    if shape == (70, 300):
        assert (want[30:40, 130:170] == 0).all() and (want[~f] != 0).all()
    # two planes at once, other widths
    wt, wf = fl.gaussian_weights(1.0, 2), fl.gaussian_weights(0.7, 0)
    v2, f2 = np.stack([v, v[::-1]]), np.stack([f, ~f])
    want = np.stack([ref.masked_gaussian_smooth(v2[i], f2[i], wt, wf) for i in range(2)])
    assert np.array_equal(fl.masked_gaussian_smooth(v2, f2, wt, wf).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- sir_operator
@pytest.mark.parametrize("axis", [-1, -2])
@pytest.mark.parametrize("L", [1, 64, 65, 1100])
def test_sir_bit_equal(fl, axis, L):
    rng = np.random.default_rng(L)
    lines = np.stack([rng.random(L) < d for d in (0.0, 1.0, 0.05, 0.3, 0.6, 0.85)] +
                     [np.repeat(rng.random(L // 8 + 1) < 0.4, 8)[:L]])            # all-clear, all-set, sparse .. dense, bursts
    f = lines if axis == -1 else np.ascontiguousarray(lines.T)
    for eta in (0.0, 0.2, 0.5):
        want = ref.sir_operator(f, eta, axis=axis)
        got = fl.sir_operator(f, eta, axis=axis)
        assert got.dtype == bool and np.array_equal(got, want), (eta, int((got != want).sum()))
        assert (want | ~f).all()
    clear, full = (fl.sir_operator(f, 0.5, axis=axis)[0], fl.sir_operator(f, 0.5, axis=axis)[1]) if axis == -1 else \
        (fl.sir_operator(f, 0.5, axis=axis)[:, 0], fl.sir_operator(f, 0.5, axis=axis)[:, 1])
    assert not clear.any() and full.all()


# ---------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def stack():
    """(8, 96, 160) complex128: the six synthetic planes, a constant plane, a plane holding a NaN and an Inf; prior flags
    with one plane flagged in full and a sprinkle on another."""
    planes, _ = synth_ref.generate(7, EVENTS, 2, 96, 160, noise=0.1, use_bandpass=False)
    data = np.concatenate([planes.reshape(6, 96, 160), np.full((1, 96, 160), 0.75 + 0j), planes[1, :1].copy()])
    data[7, 10, 10] = complex(np.nan, 0.0)
    data[7, 20, 30] = complex(0.0, np.inf)
    prior = np.zeros(data.shape, bool)
    prior[3] = True
    prior[1] = np.random.default_rng(3).random((96, 160)) < 0.01
    return data, prior


@pytest.fixture(scope="module")
def expected(stack):
    data, prior = stack
    out = {}
    for name, cfg in CONFIGS.items():
        out[name, "c128"] = ref.flag(data, **cfg)
        out[name, "c128", "prior"] = ref.flag(data, prior, **cfg)
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pipeline_complex128_stack(fl, stack, expected, name):
    data, prior = stack
    cfg = CONFIGS[name]
    x = data[:6].reshape(3, 2, 96, 160)
    got = fl.sumthreshold_flags(x, **cfg)
    assert got.dtype == bool and got.shape == x.shape
    want = expected[name, "c128"]
    assert np.array_equal(got.reshape(6, 96, 160), want[:6]), int((got.reshape(6, 96, 160) != want[:6]).sum())
    assert want[:4].any() and not want[4:6].all()
    # the whole stack: the constant plane (sigma = 0) gets no flag, NaN and Inf are flagged and the rest equals the oracle
    got = fl.sumthreshold_flags(data, **cfg)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not got[6].any() and got[7, 10, 10] and got[7, 20, 30]
    # prior flags: they stay, a plane flagged in full stays exactly that
    got = fl.sumthreshold_flags(data, flags=prior, **cfg)
    want = expected[name, "c128", "prior"]
    assert np.array_equal(got, want), int((got != want).sum())
    assert got[3].all() and (got | ~prior).all()
    assert np.array_equal(fl.sumthreshold_flags(data, flags=prior.view(np.uint8) * 7, **cfg), want)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pipeline_other_dtypes(fl, stack, name):
    data, _ = stack
    cfg = CONFIGS[name]
    sub = data[[0, 2, 7]]
    c64 = sub.astype(np.complex64)
    assert np.array_equal(fl.sumthreshold_flags(c64, **cfg), ref.flag(c64, **cfg))
    with np.errstate(invalid="ignore"):
        f64 = np.abs(sub)
    f64[0, 5, 5] = 1e300                                   # finite in float64, infinite once rounded to float32: flagged
    want = ref.flag(f64, **cfg)
    assert np.array_equal(fl.sumthreshold_flags(f64, **cfg), want) and want[0, 5, 5]
    with np.errstate(over="ignore"):
        f32 = f64.astype(np.float32)
    assert np.array_equal(fl.sumthreshold_flags(f32, **cfg), ref.flag(f32, **cfg))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pipeline_small_and_odd_planes(fl, name):
    cfg = CONFIGS[name]
    rng = np.random.default_rng(65)
    x = (1.0 + 0.1 * rng.standard_normal((2, 65, 64))).astype(np.float32)
    x[0, 30] += 1.0
    x[1, :, 7] += 0.5
    want = ref.flag(x, **cfg)
    assert np.array_equal(fl.sumthreshold_flags(x, **cfg), want) and want[0, 30].all()
    one = np.array([[3.0 + 4.0j]])
    assert fl.sumthreshold_flags(one, **cfg).tolist() == [[False]] == ref.flag(one, **cfg).tolist()
    assert fl.sumthreshold_flags(np.array([[np.inf]], np.float32), **cfg).tolist() == [[True]]


def test_pipeline_device_input_and_reproducibility(fl, stack, expected):
    from rfi_toolbox_amd.runtime import Context
    data, prior = stack
    ctx = Context.get(0)
    c64 = data.astype(np.complex64)
    host = fl.sumthreshold_flags(c64, flags=prior)
    dev = fl.sumthreshold_flags(ctx.to_device(c64), flags=ctx.to_device(prior.view(np.uint8)), out="device")
    assert dev.dtype == np.uint8 and dev.shape == c64.shape
    assert dev.numpy().tobytes() == host.view(np.uint8).tobytes()
    again = fl.sumthreshold_flags(ctx.to_device(c64), flags=ctx.to_device(prior.view(np.uint8)), out="device")
    assert again.numpy().tobytes() == dev.numpy().tobytes()
    assert fl.sumthreshold_flags(data).tobytes() == expected["defaults", "c128"].tobytes()
    assert fl.sumthreshold_flags(data).tobytes() == fl.sumthreshold_flags(data).tobytes()
    import torch
    t = torch.from_numpy(c64).cuda()
    got = fl.sumthreshold_flags(t, flags=torch.from_numpy(prior).cuda())
    assert got.is_cuda and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), host)


# ---------------------------------------------------------------------------------------------- the plane-group driver
def test_stack_across_a_group_boundary(fl):
    """The driver that carries a stack through the context's scratch, with more than one group: 2 planes of 4096 x 8192
    float32.  One plane needs 26 bytes of workspace per sample (832 MiB) and up to 5 more with host data and prior flags
    staged (992 MiB), plus the state record, the weight tables and the alignment of the regions (well under 1 MiB): one plane
    fits the 1 GiB budget and two do not, so the call takes two groups of one plane and the second starts at plane 1.  The
    reference is the single-group path (each plane flagged on its own), which the tests above pin to the NumPy oracle; no
    oracle runs at this size."""
    import torch
    C, T = 4096, 8192
    assert 31 * C * T + (1 << 20) <= 1 << 30 < 2 * 26 * C * T
    gen = torch.Generator(device="cuda").manual_seed(20)
    x = 1.0 + 0.1 * torch.randn((2, C, T), generator=gen, device="cuda", dtype=torch.float32)
    x[0, 100] += 2.0                                       # a few strong lines, other ones in each plane
    x[0, :, 5000:5003] += 2.0
    x[1, 3000:3002] += 2.0
    x[1, :, 77] += 2.0
    cfg = dict(iterations=1, levels=1, sir_eta=0.2)
    host = x.cpu().numpy()
    modes = {"cuda tensor -> host": (x, "host", lambda r: r.cpu().numpy()),
             "cuda tensor -> device": (x, "device", lambda r: r.numpy().view(bool)),
             "numpy (staged)": (host, "host", lambda r: r)}
    for name, (data, out, to_numpy) in modes.items():
        stacked = to_numpy(fl.sumthreshold_flags(data, out=out, **cfg))
        assert stacked.dtype == bool and stacked.shape == (2, C, T), name
        for i in range(2):
            alone = to_numpy(fl.sumthreshold_flags(data[i], out=out, **cfg))
            assert np.array_equal(stacked[i], alone), (name, i, int((stacked[i] != alone).sum()))
        assert stacked[0, 100].all() and stacked[1, 3000].all() and not stacked.all(), name
        assert not np.array_equal(stacked[0], stacked[1]), name      # (so equality above tells plane 1 from plane 0 flagged twice)
