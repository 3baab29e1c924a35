"""The kernels the per-epoch FID adds to metric.hip: the streamed activation statistics (gcc_activation_stats_update / _finish)
against numpy's mean / cov in float64 over the tile edges of the one-shot kernel's tests and over the ways a run can be cut into
batches, and gcc_fid_input's three input forms against util.tensor2imgs(...) / 255 on the host, bit for bit.

Tolerances of the statistics: those of tests/test_metric_kernels_gpu.py::test_activation_stats_shapes (mu rtol 1e-12 / atol 1e-13,
sigma rtol 1e-11 / atol 1e-13).  A float64 numpy restatement of the same merge over these splits at (127, 130) stays within 9e-16
of np.cov: about three orders of margin."""
import numpy as np
import pytest
import torch

from tests.test_kernels_gpu import BAD_ARG, DEV, ERR_WORKSPACE, _ops

pytestmark = pytest.mark.gpu


def _activations(rng, n, d):
    """the recipe of tests/test_metric_kernels_gpu.py::_activations (fixture_metric): anisotropic Gaussian samples in a random
    basis, a mean offset, stored as fp32"""
    basis = rng.randn(d, d) / np.sqrt(d)
    a = (rng.randn(n, d) * (0.2 + rng.rand(d))) @ basis + rng.randn(d) * 0.3
    return a.astype(np.float32)


# (n, d) at the tile edges of the one-shot kernel's cases: d below a 16-deep GEMM step, one 64 x 64 tile and a second, a third
# tile row, one column past four 64-column workgroups of the centring pass
SHAPES = [(2, 1), (2, 257), (63, 15), (64, 65), (65, 130), (127, 64), (127, 130)]


def _splits(n):
    """row by row (Welford) | one batch | a single row first | full batches and a remainder | a 64 / 63 cut, where they fit"""
    out = []
    for s in ([1] * n, [n], [1, n - 1], [50, 50, 27], [64, 63]):
        if sum(s) == n and s not in out:
            out.append(s)
    return out


def _stream(act_dev, split, d):
    from gcc_amd.metric import fid_score as F
    st = F.ActivationStream(d, max(split), DEV)
    # stale contents: the first update writes mean and m2 without reading them
    st.mean.fill_(float('nan'))
    st.m2.fill_(float('nan'))
    r = 0
    for b in split:
        st.update(act_dev[r:r + b])
        r += b
    assert st.n == r
    mu, sigma = st.result()
    return mu.cpu().numpy(), sigma.cpu().numpy()


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'f64'])
@pytest.mark.parametrize('n,d', SHAPES)
def test_streamed_stats_match_numpy_over_splits(n, d, dtype):
    act = _activations(np.random.RandomState(1000 * n + d), n, d).astype(dtype)
    a64 = act.astype(np.float64)
    mu_ref, sigma_ref = np.mean(a64, axis=0), np.cov(a64, rowvar=False).reshape(d, d)
    act_dev = torch.from_numpy(act).to(DEV)
    splits = _splits(n)
    assert len(splits) >= 2
    for split in splits:
        mu, sigma = _stream(act_dev, split, d)
        print('stream n %d d %d split %s: max |mu err| %.3g, max |sigma err| %.3g'
              % (n, d, split if len(split) < 5 else '[1] * %d' % n, np.abs(mu - mu_ref).max(), np.abs(sigma - sigma_ref).max()))
        assert np.allclose(mu, mu_ref, rtol=1e-12, atol=1e-13), split
        assert np.allclose(sigma, sigma_ref, rtol=1e-11, atol=1e-13), split


def test_streamed_stats_read_strided_rows_in_place():
    """ld > d: the rows of a wider buffer and a [b, d, 1, 1] network output, neither copied"""
    n, d = 65, 130
    act = _activations(np.random.RandomState(5), n, d)
    a64 = act.astype(np.float64)
    mu_ref, sigma_ref = np.mean(a64, axis=0), np.cov(a64, rowvar=False)
    wide = torch.full((n, d + 7), float('nan'), device=DEV)
    wide[:, :d] = torch.from_numpy(act).to(DEV)
    view = wide[:, :d]
    assert view.stride(0) == d + 7 and not view.is_contiguous()
    mu, sigma = _stream(view, [50, 15], d)
    assert np.allclose(mu, mu_ref, rtol=1e-12, atol=1e-13) and np.allclose(sigma, sigma_ref, rtol=1e-11, atol=1e-13)
    four = torch.from_numpy(act).to(DEV).view(n, d, 1, 1)
    mu, sigma = _stream(four, [64, 1], d)
    assert np.allclose(mu, mu_ref, rtol=1e-12, atol=1e-13) and np.allclose(sigma, sigma_ref, rtol=1e-11, atol=1e-13)


def test_streamed_stats_refusals_launch_nothing():
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_score as F
    ops = _ops()
    lib = ops.lib()
    b, d = 8, 33
    need = lib.gcc_activation_stats_stream_workspace(b, d)
    assert need == (b * d + d) * 8 and lib.gcc_activation_stats_stream_workspace(0, d) == 0
    act = torch.zeros((b, d), device=DEV)
    mean = torch.full((d,), 9.0, dtype=torch.float64, device=DEV)
    m2 = torch.full((d, d), 9.0, dtype=torch.float64, device=DEV)
    sigma = torch.full((d, d), 9.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    st = ops.stream()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    assert lib.gcc_activation_stats_finish(m2.data_ptr(), 1, d, sigma.data_ptr(), st) == BAD_ARG
    assert lib.gcc_activation_stats_finish(m2.data_ptr(), 0, d, sigma.data_ptr(), st) == BAD_ARG
    upd = lambda ld, bb, n_before, nbytes: lib.gcc_activation_stats_update(act.data_ptr(), 0, ld, bb, d, n_before, mean.data_ptr(),
                                                                           m2.data_ptr(), ws.data_ptr(), nbytes, st)
    assert upd(d, b, 0, need - 1) == ERR_WORKSPACE
    assert upd(d, b, 0, lib.gcc_activation_stats_stream_workspace(b - 1, d)) == ERR_WORKSPACE
    assert upd(d - 1, b, 0, need) == BAD_ARG            # rows that overlap
    assert upd(d, 0, 0, need) == BAD_ARG
    assert upd(d, b, -1, need) == BAD_ARG
    assert int(lib.gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    assert bool((mean == 9.0).all()) and bool((m2 == 9.0).all()) and bool((sigma == 9.0).all())
    s = F.ActivationStream(d, b, DEV)
    s.update(act[:1])
    with pytest.raises(GccError, match='at least 2'):
        s.result()
    with pytest.raises(GccError, match='1..8'):
        s.update(torch.zeros((b + 1, d), device=DEV))


# ---- gcc_fid_input --------------------------------------------------------------------------------------------------------
def _host(x_nchw):
    """util.tensor2imgs(x) / 255 as metric/fid_score.py:184-190 feeds it: float64 division, then FloatTensor; NCHW"""
    from gcc_amd.utils import util
    bytes_ = util.tensor2imgs(x_nchw)                                            # uint8 [N, H, W, 3]
    return bytes_, np.ascontiguousarray(np.transpose(bytes_.astype(np.float64) / 255, (0, 3, 1, 2)).astype(np.float32))


def _as_planes(values):
    """a flat list of fp32 values as an NCHW [1, 3, 1, W] image, zero-padded"""
    v = np.asarray(values, dtype=np.float32)
    v = np.concatenate([v, np.zeros((-len(v)) % 3, dtype=np.float32)])
    return torch.from_numpy(v).view(1, 3, 1, -1)


def _nhwc(x):
    ops = _ops()
    N, _, H, W = x.shape
    xd = ops.new_act(N, 3, H, W, DEV)
    ops.nchw_to_nhwc(x.to(DEV).contiguous(), xd)
    return xd


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fid_input_bf16_form_every_value_in_range():
    from gcc_amd.metric import fid_eval as E
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16).float()
    v = v[torch.isfinite(v) & (v.abs() <= 1)]
    assert v.numel() == 2 * (0x3F80 + 1)                                          # +-0 .. +-1
    x = _as_planes(np.concatenate([v.numpy(), np.float32([-3.0, 3.0, 1.0078125, -1.0078125])]))
    bytes_, want = _host(x)
    assert len(np.unique(bytes_)) == 256
    got = E.fid_input(_nhwc(x)).cpu().numpy()
    assert _same_bits(got, want)


def test_fid_input_fp32_form_loader_values_and_byte_boundaries():
    from gcc_amd.metric import fid_eval as E
    b = torch.arange(256, dtype=torch.float32)
    loader = ((b / 255.0 - 0.5) / 0.5).numpy()                                    # ToTensor + Normalize(.5, .5), fp32
    edge = (2.0 * np.arange(1, 256, dtype=np.float64) / 255.0 - 1.0).astype(np.float32)      # (x + 1) / 2 * 255 == b near here
    lo, hi = np.nextafter(edge, np.float32(-2)), np.nextafter(edge, np.float32(2))
    ends = np.float32([-1.0, 1.0])
    outside = np.float32([-1.5, 1.5, 100.0, -100.0, 3e38, -3e38, np.nextafter(np.float32(1), np.float32(2)),
                          np.nextafter(np.float32(-1), np.float32(-2)), 1.0078125, -0.0])
    x = _as_planes(np.concatenate([loader, ends, lo, edge, hi, np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(2)),
                                   outside]))
    bytes_, want = _host(x)
    flat = np.transpose(bytes_, (0, 3, 1, 2)).reshape(-1)
    drift = flat[:256].astype(int) - np.arange(256)
    print('loader round trip: %d of 256 bytes come back one lower' % int((drift == -1).sum()))
    assert set(drift.tolist()) == {0, -1} and int((drift == -1).sum()) == 63
    got = E.fid_input(x.to(DEV)).cpu().numpy()
    assert _same_bits(got, want)


def test_fid_input_u8_form_every_byte():
    from gcc_amd.metric import fid_eval as E
    b = np.arange(256, dtype=np.uint8)
    img = np.stack([b, np.roll(b, 85), np.roll(b, 170)], axis=-1).reshape(1, 16, 16, 3)
    want = np.ascontiguousarray(np.transpose(img.astype(np.float64) / 255, (0, 3, 1, 2)).astype(np.float32))
    got = E.fid_input(torch.from_numpy(img).to(DEV)).cpu().numpy()
    assert _same_bits(got, want)
    one = E.fid_input(torch.from_numpy(img[0]).to(DEV)).cpu().numpy()              # [h, w, 3] is one image
    assert _same_bits(one, want)


# (3, 5, 7): 315 elements, a tail below one workgroup and no whole float4 run; (2, 64, 64): several workgroups, the float4 path
@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 64, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_fid_input_shapes_all_forms(shape):
    from gcc_amd.metric import fid_eval as E
    N, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    x = (torch.rand(N, 3, H, W, generator=g) * 2.2 - 1.1)
    bytes_, want = _host(x)
    assert _same_bits(E.fid_input(x.to(DEV)).cpu().numpy(), want)
    xb = x.bfloat16().float()
    assert _same_bits(E.fid_input(_nhwc(xb)).cpu().numpy(), _host(xb)[1])
    assert _same_bits(E.fid_input(torch.from_numpy(bytes_).to(DEV)).cpu().numpy(), want)


@pytest.mark.parametrize('form', ['fp32', 'bf16', 'u8'])
def test_fid_input_writes_one_slot_of_a_batch_buffer(form):
    from gcc_amd.metric import fid_eval as E
    H, W = 5, 7                                   # a slot of 105 floats: slot 2 starts 840 bytes in (8-byte, not 16-byte aligned)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(1, 3, H, W, generator=g) * 2 - 1).bfloat16().float()
    bytes_, want = _host(x)
    src = {'fp32': lambda: x.to(DEV), 'bf16': lambda: _nhwc(x), 'u8': lambda: torch.from_numpy(bytes_).to(DEV)}[form]()
    buf = torch.full((4, 3, H, W), 7.0, device=DEV)
    out = E.fid_input(src, buf[2:3])
    assert out.data_ptr() == buf[2].data_ptr()
    got = buf.cpu().numpy()
    assert _same_bits(got[2:3], want)
    assert (got[:2] == 7.0).all() and (got[3:] == 7.0).all()
