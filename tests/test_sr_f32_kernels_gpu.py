"""The two streaming kernels at the output end of SRGAN's fp32 inference route: gcc_nhwc_f32_to_nchw_f32 (the image into the NCHW
buffer the metric kernels read) is a copy and must be exact; gcc_image_to_u8_f32 must give the byte of the reference's
util.tensor2im, ((x + 1) / 2 * 255).astype(uint8) in fp32 on the host, at both fp32 neighbours of every byte boundary."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG = -1
SENTINEL = -77.25


@pytest.mark.parametrize('ld', [4, 8])
@pytest.mark.parametrize('N,H,W', [(1, 5, 7), (2, 48, 40)])
def test_nhwc_f32_to_nchw_f32_is_exact(N, H, W, ld):
    from gcc_amd import ops
    g = torch.Generator().manual_seed(N * 100 + H + ld)
    src = torch.randn((N, H, W, ld), generator=g)
    view = src.to(DEV).permute(0, 3, 1, 2)[:, :3]
    out = torch.full((N * 3 * H * W + 16,), SENTINEL, dtype=torch.float32, device=DEV)
    got = ops.nhwc_to_nchw_f32(view, out[:N * 3 * H * W])
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().view(N, 3, H, W).view(torch.int32), src[..., :3].permute(0, 3, 1, 2).contiguous().view(torch.int32))
    assert (out[N * 3 * H * W:] == SENTINEL).all()
    if ld == 8:                    # a channel window inside the pixel: off = 4
        L = ops.lib()
        assert L.gcc_nhwc_f32_to_nchw_f32(view.data_ptr(), out.data_ptr(), N, 3, H, W, ld, 4, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:N * 3 * H * W].cpu().view(N, 3, H, W), src[..., 4:7].permute(0, 3, 1, 2).contiguous())


def test_nhwc_f32_to_nchw_f32_refusals():
    from gcc_amd import ops
    L = ops.lib()
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = t.data_ptr()
    L.gcc_launch_count(1)
    assert L.gcc_nhwc_f32_to_nchw_f32(None, p, 1, 3, 2, 2, 4, 0, None) == BAD_ARG
    assert L.gcc_nhwc_f32_to_nchw_f32(p, None, 1, 3, 2, 2, 4, 0, None) == BAD_ARG
    assert L.gcc_nhwc_f32_to_nchw_f32(p, p + 128, 1, 3, 2, 2, 4, 4, None) == BAD_ARG           # the window outside its ld
    assert L.gcc_nhwc_f32_to_nchw_f32(p, p + 128, 0, 3, 2, 2, 4, 0, None) == BAD_ARG
    assert L.gcc_launch_count(0) == 0


def _tensor2im(a):
    return ((a + np.float32(1)) / np.float32(2.0) * np.float32(255.0)).astype(np.uint8)


def test_image_to_u8_f32_matches_tensor2im_at_every_byte_boundary():
    """for every byte b the fp32 x nearest to 2 b / 255 - 1 and five fp32 neighbours on either side (the boundary of the
    truncation lies among them), -1 and 1 and their neighbours inside, and values outside [-1, 1], which the reference clamps
    beforehand (tanh never produces them; the kernel clamps to 0 / 255)"""
    from gcc_amd import ops
    b = np.arange(0, 257, dtype=np.float64)
    centre = (2.0 * b / 255.0 - 1.0).astype(np.float32)
    vals = [centre]
    up, dn = centre.copy(), centre.copy()
    for _ in range(5):
        up, dn = np.nextafter(up, np.float32(2)), np.nextafter(dn, np.float32(-2))
        vals += [up.copy(), dn.copy()]
    inside = np.concatenate(vals)
    inside = inside[(inside >= -1) & (inside <= 1)]
    edge = np.array([-1.0, 1.0, np.nextafter(np.float32(-1), np.float32(0)), np.nextafter(np.float32(1), np.float32(0)), 0.0, -0.0],
                    dtype=np.float32)
    outside = np.array([-1.0000001, 1.0000001, -1.5, 1.5, -100.0, 100.0, 3e38, -3e38], dtype=np.float32)
    x = np.concatenate([inside, edge, outside]).astype(np.float32)
    x = np.concatenate([x, np.zeros((-len(x)) % 3, dtype=np.float32)])
    P = len(x) // 3
    for ld in (4, 8):
        buf = torch.full((1, 1, P, ld), 0.5, dtype=torch.float32)
        buf[0, 0, :, :3] = torch.from_numpy(x).view(P, 3)
        view = buf.to(DEV).permute(0, 3, 1, 2)[:, :3]
        got = ops.image_to_u8(view).cpu().numpy().reshape(-1)
        want = _tensor2im(np.clip(x, -1, 1))
        assert got.dtype == np.uint8 and np.array_equal(got, want), (ld, x[got != want][:5], got[got != want][:5], want[got != want][:5])
    n_in = len(inside) + len(edge)
    assert np.array_equal(got[:n_in], _tensor2im(x[:n_in]))             # inside [-1, 1] no clamp is involved
    assert set(np.unique(got[:len(inside)])) == set(range(256))         # every byte is reached


def test_image_to_u8_f32_refusals():
    from gcc_amd import ops
    L = ops.lib()
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    o = torch.zeros(64, dtype=torch.uint8, device=DEV)
    L.gcc_launch_count(1)
    assert L.gcc_image_to_u8_f32(None, 4, 0, 4, o.data_ptr(), None) == BAD_ARG
    assert L.gcc_image_to_u8_f32(t.data_ptr(), 4, 0, 4, None, None) == BAD_ARG
    assert L.gcc_image_to_u8_f32(t.data_ptr(), 4, 4, 4, o.data_ptr(), None) == BAD_ARG
    assert L.gcc_image_to_u8_f32(t.data_ptr(), 4, 0, 0, o.data_ptr(), None) == 0            # no pixels: nothing to do
    assert L.gcc_launch_count(0) == 0
