"""The evaluation kernels of metric.hip at the sizes where their loops change shape: gcc_psnr_y_sse and gcc_ssim_y_sum (smallest
legal images, up to 1024 partials and a grid-stride trip), gcc_activation_stats and gcc_frechet_distance (d below a tile, a third
tile row, d past one workgroup of columns, the n = 64 / 65 edge of the row split, rank-deficient covariances), gcc_argmax_channels
and gcc_confusion_hist (C = 1, -inf and all-equal pixels, a grid-stride trip, the largest table that fits the LDS).

References: oracle.metric_oracle (the CPU restatement of the reference's arithmetic) and numpy in float64.  Tolerances are those of
tests/test_metric.py, which keeps its one-size tests: 1e-5 relative on the PSNR sum, 1e-9 absolute on mean SSIM, 1e-12 on
ssim(x, x), rtol 1e-12 / 1e-11 on mu / sigma, 1e-7 relative on the Frechet distance; integer results are exact."""
import numpy as np
import pytest
import torch

from tests.test_kernels_gpu import BAD_ARG, DEV, ERR_WORKSPACE, _ops

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2                  # include/gcc_hip.h GCC_ERR_UNSUPPORTED


# ---- PSNR / SSIM ----------------------------------------------------------------------------------------------------------
# (N, H, W): the smallest legal PSNR image (one pixel left of the crop) | the smallest SSIM image (one window) | a strip one
# window high | odd sizes | 522 x 522 = 272484 cropped pixels and 516 x 516 = 266256 window centres: just past 1024 workgroups x 256,
# the first to walk the grid-stride loop twice | about 2.5 times that with N = 2 (a third trip)
SR_SIZES = [(1, 9, 9), (1, 15, 15), (3, 15, 40), (2, 23, 17), (1, 530, 530), (2, 570, 600)]


def _sr_pair(N, H, W):
    """as tests/golden/make_fixtures.py::fixture_metric: fake uniform in [-1, 1], real = fake + 0.1-sigma noise, clamped"""
    g = torch.Generator().manual_seed(78 + H * 1000 + W)
    fake = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    real = (fake + 0.1 * torch.randn(N, 3, H, W, generator=g)).clamp(-1, 1)
    return fake, real


def _y_kernel_order(img):
    """the luminance in the kernel's own order (metric.hip luma): r * 65.481 rounded, g * 128.553 fused into it, b * 24.966 fused
    into that, / 255 + 16, each in fp32.  A fused multiply-add is restated as the float64 product (exact: 2 x 24 bits) and sum,
    rounded to fp32.  oracle.metric_oracle.y_channel leaves the order to numpy's matmul: the same bits on images of more than one
    pixel, another last bit on the single pixel of the 9 x 9 case (there the oracle is 9.5e-6 from this restatement and from the
    kernel: nearly the whole 1e-5)"""
    x = np.float32(255.) * ((img.astype(np.float32) + np.float32(1.)) / np.float32(2.))[:, :, 4:-4, 4:-4]
    r, g, b = (x[:, c].astype(np.float64) for c in range(3))
    cr, cg, cb = (float(np.float32(v)) for v in (65.481, 128.553, 24.966))
    t = (r * cr).astype(np.float32).astype(np.float64)
    t = (g * cg + t).astype(np.float32).astype(np.float64)
    t = (b * cb + t).astype(np.float32)
    return t / np.float32(255.) + np.float32(16.)


def _sr_call(fn_name, fake, real, out, accumulate, ws, ws_bytes=None):
    ops = _ops()
    N, _, H, W = fake.shape
    return getattr(ops.lib(), fn_name)(fake.data_ptr(), real.data_ptr(), N, H, W, out.data_ptr(), accumulate, ws.data_ptr(),
                                       ws.numel() if ws_bytes is None else ws_bytes, ops.stream())


@pytest.mark.parametrize('size', SR_SIZES, ids=lambda s: 'x'.join(map(str, s)))
def test_psnr_y_sse_sizes(size):
    from oracle import metric_oracle as M
    ops = _ops()
    fake, real = _sr_pair(*size)
    ref = float(np.sum((M.y_channel(fake.numpy()).astype(np.float64) - M.y_channel(real.numpy()).astype(np.float64)) ** 2))
    fd, rd = fake.to(DEV), real.to(DEV)
    ws = torch.empty(ops.lib().gcc_psnr_workspace(), dtype=torch.uint8, device=DEV)
    sse = torch.full((1,), 9.0, dtype=torch.float64, device=DEV)              # stale contents: accumulate = 0 overwrites
    assert _sr_call('gcc_psnr_y_sse', fd, rd, sse, 0, ws) == 0
    first = sse.item()
    print('psnr sse %s: %.12g, oracle %.12g, rel err %.3g (limit 1e-5)' % (size, first, ref, abs(first - ref) / ref))
    assert abs(first - ref) <= 1e-5 * ref
    own = float(np.sum((_y_kernel_order(fake.numpy()).astype(np.float64) - _y_kernel_order(real.numpy()).astype(np.float64)) ** 2))
    print('psnr sse %s: against the luminance restated in the kernel\'s order %.12g, rel err %.3g' % (size, own, abs(first - own) / own))
    assert abs(first - own) <= 1e-5 * own
    assert _sr_call('gcc_psnr_y_sse', fd, rd, sse, 1, ws) == 0
    assert sse.item() == 2 * first, 'accumulate: a fixed-order sum added to itself'
    assert _sr_call('gcc_psnr_y_sse', rd, rd, sse, 0, ws) == 0
    assert sse.item() == 0.0, 'psnr(real, real): both images go through one luminance arithmetic'
    N, H, W = size
    psnr = 10 * np.log10(255. ** 2 / (first / (N * (H - 8) * (W - 8))))
    assert abs(psnr - M.psnr_y(fake.numpy(), real.numpy())) < 1e-4


@pytest.mark.parametrize('size', SR_SIZES[1:], ids=lambda s: 'x'.join(map(str, s)))
def test_ssim_y_sum_sizes(size):
    from oracle import metric_oracle as M
    ops = _ops()
    N, H, W = size
    fake, real = _sr_pair(*size)
    ref = M.ssim_y(fake.numpy(), real.numpy())
    fd, rd = fake.to(DEV), real.to(DEV)
    ws = torch.empty(ops.lib().gcc_psnr_workspace(), dtype=torch.uint8, device=DEV)
    acc = torch.full((1,), 9.0, dtype=torch.float64, device=DEV)
    assert _sr_call('gcc_ssim_y_sum', fd, rd, acc, 0, ws) == 0
    first = acc.item()
    count = N * (H - 14) * (W - 14)
    print('ssim %s: %.12g, oracle %.12g, err %.3g (limit 1e-9)' % (size, first / count, ref, abs(first / count - ref)))
    assert 0.0 < ref < 1.0 and abs(first / count - ref) < 1e-9
    assert _sr_call('gcc_ssim_y_sum', fd, rd, acc, 1, ws) == 0
    assert acc.item() == 2 * first, 'accumulate'
    assert _sr_call('gcc_ssim_y_sum', rd, rd, acc, 0, ws) == 0
    assert abs(acc.item() / count - 1.0) < 1e-12, 'ssim(real, real)'


def test_psnr_ssim_refusals_launch_nothing():
    ops = _ops()
    lib = ops.lib()
    need = lib.gcc_psnr_workspace()
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.full((1,), 9.0, dtype=torch.float64, device=DEV)
    img = torch.zeros(1, 3, 16, 16, device=DEV)
    p, st = img.data_ptr(), ops.stream()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    assert lib.gcc_psnr_y_sse(p, p, 1, 8, 16, out.data_ptr(), 0, ws.data_ptr(), need, st) == BAD_ARG          # nothing left of the crop
    assert lib.gcc_psnr_y_sse(p, p, 1, 16, 8, out.data_ptr(), 0, ws.data_ptr(), need, st) == BAD_ARG
    assert lib.gcc_ssim_y_sum(p, p, 1, 14, 16, out.data_ptr(), 0, ws.data_ptr(), need, st) == BAD_ARG         # no whole window
    assert lib.gcc_ssim_y_sum(p, p, 1, 16, 14, out.data_ptr(), 0, ws.data_ptr(), need, st) == BAD_ARG
    assert lib.gcc_psnr_y_sse(p, p, 1, 16, 16, out.data_ptr(), 0, ws.data_ptr(), need - 1, st) == ERR_WORKSPACE
    assert lib.gcc_ssim_y_sum(p, p, 1, 16, 16, out.data_ptr(), 0, ws.data_ptr(), need - 1, st) == ERR_WORKSPACE
    assert int(lib.gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    assert out.item() == 9.0


# ---- activation statistics / Frechet distance -----------------------------------------------------------------------------
def _activations(rng, n, d, transpose=False):
    """as fixture_metric: anisotropic Gaussian samples in a random basis, a mean offset, stored as fp32"""
    basis = rng.randn(d, d) / np.sqrt(d)
    a = (rng.randn(n, d) * (0.2 + rng.rand(d))) @ (basis.T if transpose else basis) + rng.randn(d) * 0.3
    return a.astype(np.float32)


# n: 2 (the least) | 63 (one slice) | 64, 65 (64 slices of 1 and of 2 rows: with 65, slices 33..63 start past the end) | 127
# d: 1, 15 (below a 16-deep GEMM step) | 63, 64, 65 (one 64 x 64 tile and a second) | 130 (a third tile row) | 257 (one column past
# a workgroup of colsum_kernel / mean_finalize_kernel)
STATS_CASES = [(2, 1), (2, 257), (63, 15), (63, 64), (64, 65), (64, 257), (65, 63), (65, 130), (127, 64), (127, 130), (127, 1)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'f64'])
@pytest.mark.parametrize('n,d', STATS_CASES)
def test_activation_stats_shapes(n, d, dtype):
    from gcc_amd.metric import fid_score as F
    act = _activations(np.random.RandomState(1000 * n + d), n, d).astype(dtype)
    a64 = act.astype(np.float64)
    mu_ref, sigma_ref = np.mean(a64, axis=0), np.cov(a64, rowvar=False).reshape(d, d)
    mu, sigma = F.activation_statistics(act)
    mu, sigma = mu.cpu().numpy(), sigma.cpu().numpy()
    print('stats n %d d %d: max |mu err| %.3g, max |sigma err| %.3g' % (n, d, np.abs(mu - mu_ref).max(), np.abs(sigma - sigma_ref).max()))
    assert np.allclose(mu, mu_ref, rtol=1e-12, atol=1e-13)
    assert np.allclose(sigma, sigma_ref, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize('rank', ['full', 'deficient'])
@pytest.mark.parametrize('d', [15, 65, 130])
def test_frechet_distance_shapes(d, rank):
    """full rank: 4 d and 3 d samples; rank-deficient: fewer samples than dimensions in both sets (singular covariance product)"""
    from gcc_amd.metric import fid_score as F
    from oracle import metric_oracle as M
    rng = np.random.RandomState(77 + d)
    n1, n2 = (4 * d, 3 * d) if rank == 'full' else (d // 2 + 1, (2 * d) // 3)
    a1, a2 = _activations(rng, n1, d), _activations(rng, n2, d, transpose=True)
    m1, s1 = M.activation_statistics(a1)
    m2, s2 = M.activation_statistics(a2)
    ref = float(M.calculate_frechet_distance(m1, s1, m2, s2))
    mu1, sg1 = F.activation_statistics(a1)
    mu2, sg2 = F.activation_statistics(a2)
    fid, resid = F.calculate_frechet_distance(mu1, sg1, mu2, sg2, return_residual=True)
    print('frechet d %d %s: %.12g reference %.12g (rel %.2e), last Newton-Schulz step moved the trace by %.1e' % (
        d, rank, fid, ref, abs(fid - ref) / ref, resid))
    assert abs(fid - ref) <= 1e-7 * ref, (fid, ref)
    own = F.calculate_frechet_distance(m1, s1, m1, s1)
    print('frechet d %d %s: distance to itself %.3g, 2 tr(sigma) %.4g' % (d, rank, own, 2 * np.trace(s1)))
    assert abs(own) < 1e-6 * 2 * np.trace(s1)


# ---- argmax / confusion matrix --------------------------------------------------------------------------------------------
# (N, C, H, W); the last: 2098176 pixels, past 8192 workgroups x 256
@pytest.mark.parametrize('shape', [(2, 1, 5, 7), (2, 5, 7, 9), (1, 3, 1024, 2049)], ids=lambda s: 'x'.join(map(str, s)))
def test_argmax_channels_edges(shape):
    from gcc_amd.metric import mIoU_score as G
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(H + W)
    s = torch.randn(N, Cc, H, W, generator=g)
    s[0, :, 0, 1] = float('-inf')                        # every score -inf: index 0
    s[N - 1, :, H - 1, W - 2] = 0.25                     # all equal: the first
    s[N - 1, :, H - 1, W - 1] = float('-inf')            # the very last pixel
    if Cc > 1:
        s[0, 0, 1, 2] = float('-inf')                    # -inf in front of finite scores
        s[0, Cc - 1, 2, 3] = s[0, :, 2, 3].max() + 1     # the last class wins
    pred = G.argmax_classes(s.to(DEV)).cpu().numpy()
    ref = s.numpy().argmax(axis=1)
    assert ref[0, 0, 1] == 0 and ref[N - 1, H - 1, W - 2] == 0
    assert pred.dtype == np.int32 and np.array_equal(pred, ref)


def _hist_inputs(n, count, seed):
    """labels in [-2, n + 5) and 255 (ignored outside [0, n)), predictions in [-3, n + 4): those outside [0, n) are dropped"""
    rng = np.random.RandomState(seed)
    label = rng.randint(-2, n + 5, size=count).astype(np.int32)
    label[rng.rand(count) < 0.05] = 255
    pred = rng.randint(-3, n + 4, size=count).astype(np.int32)
    return pred, label


def _hist_reference(pred, label, n):
    from oracle import metric_oracle as M
    ok = (pred >= 0) & (pred < n)                        # hist_kernel counts a pixel only where 0 <= pred < n as well
    return M.fast_hist(pred[ok].astype(np.int64), label[ok].astype(np.int64), n)


@pytest.mark.parametrize('n,count', [(110, 300_000), (110, 1), (19, 257), (1, 1000)])
def test_confusion_hist_edges(n, count):
    """n = 110: 48400 bytes of counters, the largest table the 48 KB of LDS take"""
    from gcc_amd.metric import mIoU_score as G
    pred, label = _hist_inputs(n, count, n + count)
    if count > 1000:
        assert (pred < 0).any() and (pred >= n).any() and (label == n - 1).any() and (pred == n - 1).any()
    ref = _hist_reference(pred, label, n)
    hist = G.fast_hist(pred, label, n)
    assert hist.dtype == torch.int64 and np.array_equal(hist.cpu().numpy(), ref)
    hist = G.fast_hist(pred, label, n, hist)
    assert np.array_equal(hist.cpu().numpy(), 2 * ref), 'accumulates'


def test_confusion_hist_refusals_and_empty_input():
    ops = _ops()
    lib = ops.lib()
    pred, label = _hist_inputs(19, 64, 3)
    pd, ld = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    hist = torch.full((111 * 111,), 5, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    assert lib.gcc_confusion_hist(pd.data_ptr(), ld.data_ptr(), 64, 111, hist.data_ptr(), ops.stream()) == UNSUPPORTED
    assert lib.gcc_confusion_hist(pd.data_ptr(), ld.data_ptr(), 0, 19, hist.data_ptr(), ops.stream()) == 0      # count 0: nothing to do
    assert lib.gcc_confusion_hist(pd.data_ptr(), ld.data_ptr(), 64, 0, hist.data_ptr(), ops.stream()) == BAD_ARG
    assert int(lib.gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    assert bool((hist == 5).all())
