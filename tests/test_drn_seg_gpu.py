"""The native DRN-D segmenter on the GPU: gcc_phase_regroup and gcc_relu_bf16 bit for bit, gcc_seg_head against torch-CPU fp32,
whole nets against the reference's fp32 results (tests/golden/drn_seg.npz) within twice the error of the bf16-emulating host
restatement, the reference's own --drn_path file end to end through gcc_amd.test and gcc_amd.train, and the full-width
DRN-D-105 once (launch count, memory)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gcc_oracle as O
from tests import _drn_emul as E
from tests import _miou_emul as ME
from tests.golden.recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope='module')
def z():
    return np.load(E.GOLDEN)


def _bits(shape, seed):
    """bf16 tensor of arbitrary finite bit patterns (a permutation must move bits, not values)"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 1 << 16, shape, generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7f80) == 0x7f80, b & 0x807f, b)              # no Inf / NaN: torch.equal compares values
    return b.to(torch.int16).view(torch.bfloat16)


def _phase_nhwc(x, d):
    """[N, H, W, C] logical -> [N d^2, H / d, W / d, C] by torch indexing"""
    N, H, W, Cc = x.shape
    return x.reshape(N, H // d, d, W // d, d, Cc).permute(0, 2, 4, 1, 3, 5).reshape(N * d * d, H // d, W // d, Cc)


# ---- 1. gcc_phase_regroup -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,H,W', [(2, 8, 12), (1, 4, 4)])
@pytest.mark.parametrize('Cc,ld,off', [(8, 8, 0), (24, 32, 8), (20, 32, 8)])
def test_phase_regroup_bit_exact(N, H, W, Cc, ld, off):
    from gcc_amd import ops
    L = ops.lib()
    logical = _bits((N, H, W, Cc), N * 1000 + Cc)
    sentinel = _bits((N * H * W * ld,), 77)
    C8 = ops.ceil8(Cc)
    for ds in (1, 2, 4):
        for dd in (1, 2, 4):
            if ds == dd:
                continue
            src = sentinel.clone().view(N * ds * ds, H // ds, W // ds, ld)
            src[..., off:off + Cc] = _phase_nhwc(logical, ds)
            src, dst = src.to(DEV), sentinel.flip(0).contiguous().view(N * dd * dd, H // dd, W // dd, ld).to(DEV)
            before = dst.cpu().clone()
            rc = L.gcc_phase_regroup(src.data_ptr(), ld, off, ds, dst.data_ptr(), ld, off, dd, N, H, W, Cc, None)
            assert rc == 0, (ds, dd, rc)
            got = dst.cpu()
            assert torch.equal(got[..., off:off + Cc].view(torch.int16), _phase_nhwc(logical, dd).view(torch.int16)), (ds, dd)
            assert (got[..., off + Cc:off + C8].view(torch.int16) == 0).all()                  # pad channels of the window
            keep = torch.ones(ld, dtype=torch.bool)
            keep[off:off + C8] = False
            assert torch.equal(got[..., keep].view(torch.int16), before[..., keep].view(torch.int16)), (ds, dd)   # neighbours
            # there and back is the identity
            back = sentinel.clone().view(N * ds * ds, H // ds, W // ds, ld).to(DEV)
            assert L.gcc_phase_regroup(dst.data_ptr(), ld, off, dd, back.data_ptr(), ld, off, ds, N, H, W, Cc, None) == 0
            assert torch.equal(back.cpu()[..., off:off + Cc].view(torch.int16), src.cpu()[..., off:off + Cc].view(torch.int16))
    # the wrapper on activation views
    a = ops.new_act(N, Cc, H, W, DEV, ld=ld)
    a.permute(0, 2, 3, 1).copy_(logical.to(DEV))
    b = ops.new_act(N * 4, Cc, H // 2, W // 2, DEV)
    ops.phase_regroup(a, b, 1, 2)
    assert torch.equal(b.permute(0, 2, 3, 1).cpu().view(torch.int16), _phase_nhwc(logical, 2).view(torch.int16))


def test_phase_regroup_and_relu_refuse_bad_arguments_without_a_launch():
    from gcc_amd import ops
    L = ops.lib()
    x = torch.zeros(2 * 8 * 12 * 32, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros_like(x)
    xp, yp = x.data_ptr(), y.data_ptr()
    L.gcc_launch_count(1)
    call = lambda *a: L.gcc_phase_regroup(*a, None)
    assert call(None, 32, 0, 1, yp, 32, 0, 2, 2, 8, 12, 8) == BAD_ARG
    assert call(xp, 32, 0, 1, None, 32, 0, 2, 2, 8, 12, 8) == BAD_ARG
    assert call(xp, 30, 0, 1, yp, 32, 0, 2, 2, 8, 12, 8) == BAD_ARG           # ld no multiple of 8
    assert call(xp, 32, 4, 1, yp, 32, 0, 2, 2, 8, 12, 8) == BAD_ARG           # offset no multiple of 8
    assert call(xp, 32, 0, 1, yp, 32, 16, 2, 2, 8, 12, 24) == BAD_ARG         # the window does not fit its ld
    assert call(xp, 32, 0, 1, yp, 32, 0, 2, 0, 8, 12, 8) == BAD_ARG
    assert call(xp, 32, 0, 1, yp, 32, 0, 2, 2, 8, 12, 0) == BAD_ARG
    assert call(xp, 32, 0, 1, xp, 32, 8, 2, 2, 8, 12, 8) == BAD_ARG           # never in place
    assert call(xp, 32, 0, 1, xp + 64, 32, 0, 2, 1, 8, 12, 8) == BAD_ARG      # overlapping ranges
    assert call(xp, 32, 0, 3, yp, 32, 0, 1, 2, 8, 12, 8) == UNSUPPORTED
    assert call(xp, 32, 0, 1, yp, 32, 0, 8, 2, 8, 16, 8) == UNSUPPORTED
    assert call(xp, 32, 0, 1, yp, 32, 0, 4, 2, 8, 10, 8) == UNSUPPORTED       # W no multiple of 4
    assert call(xp, 32, 0, 2, yp, 32, 0, 1, 2, 7, 12, 8) == UNSUPPORTED
    relu = lambda *a: L.gcc_relu_bf16(*a, None)
    assert relu(None, 32, 0, 8, 10) == BAD_ARG
    assert relu(xp, 32, 4, 8, 10) == BAD_ARG
    assert relu(xp, 20, 0, 8, 10) == BAD_ARG
    assert relu(xp, 32, 16, 24, 10) == BAD_ARG
    assert relu(xp, 32, 0, 8, 0) == BAD_ARG
    head = lambda *a: L.gcc_seg_head(*a, None)
    f = torch.zeros(19 * 64, dtype=torch.float32, device=DEV)
    fp = f.data_ptr()
    assert head(xp, 16, 0, 1, 2, 2, 16, fp, fp, 19, fp, None, fp) == BAD_ARG                # no scores
    assert head(xp, 16, 0, 1, 2, 2, 16, None, fp, 19, fp, fp, fp) == BAD_ARG                # no seg weights
    assert head(None, 0, 0, 1, 2, 2, 0, None, None, 19, None, fp, fp) == BAD_ARG            # log-softmax without up weights
    assert head(None, 0, 0, 1, 2, 2, 0, None, None, 19, None, fp, None) == BAD_ARG          # nothing to do
    assert head(xp, 8, 0, 1, 2, 2, 16, fp, fp, 19, fp, fp, None) == BAD_ARG                 # ld below Cin
    assert head(xp, 16, 0, 1, 2, 2, 12, fp, fp, 19, fp, fp, None) == UNSUPPORTED            # Cin no multiple of 8
    assert head(xp, 16, 0, 1, 2, 2, 16, fp, fp, 65, fp, fp, None) == UNSUPPORTED            # more than 64 classes
    assert L.gcc_launch_count(0) == 0
    assert (x == 0).all() and (y == 0).all()


# ---- 2. gcc_relu_bf16 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cc,ld,off,pixels', [(16, 32, 8, 333), (20, 32, 8, 70000), (8, 8, 0, 1)])
def test_relu_bit_exact(Cc, ld, off, pixels):
    from gcc_amd import ops
    x = _bits((pixels, ld), Cc + pixels)
    x[0, off:off + 4] = torch.tensor([-0.0, 0.0, -1.0, 2.5], dtype=torch.bfloat16)
    want = x.clone()
    w = want[:, off:off + Cc]
    want[:, off:off + Cc] = torch.where(w.float() > 0, w, torch.zeros_like(w))          # -0.0 and negatives become +0.0
    d = x.to(DEV)
    assert ops.lib().gcc_relu_bf16(d.data_ptr(), ld, off, Cc, pixels, None) == 0
    assert torch.equal(d.cpu().view(torch.int16), want.view(torch.int16))               # the window, and nothing around it
    assert d.cpu()[0, off].view(torch.int16).item() == 0


# ---- 3. gcc_seg_head on the fixtures' own scores ----------------------------------------------------------------------------------
def _head_bar(scores):
    """64 fp32 ulps of max |score| + ln C: four products and three adds of the taps, a max, C exps, a sum, a log and a subtract,
    with device exp / log good to 2 ulps"""
    return 64 * float(np.spacing(np.float32(float(scores.abs().max()) + np.log(scores.shape[1]))))


@pytest.mark.parametrize('case', ['2x19x8x12', '1x19x1x1'])
def test_seg_head_up_logsoftmax_against_torch_fp32(z, case):
    from gcc_amd import ops
    sd, _ = E.fixture_net(z, 'bneck')
    scores = torch.from_numpy(z['bneck.scores'])
    assert tuple(scores.shape) == (2, 19, 8, 12)
    if case == '1x19x1x1':                                   # every tap meets the border
        scores = scores[:1, :, 3:4, 5:6].contiguous()
    N, Cc, h, w = scores.shape
    up = sd['up.weight']
    want = E.head(scores, up)
    sc = scores.to(DEV)
    logp = torch.empty((N, Cc, 8 * h, 8 * w), dtype=torch.float32, device=DEV)
    ops.seg_head(None, None, None, up.reshape(Cc, 256).contiguous().to(DEV), sc, logp)
    got = logp.cpu()
    assert torch.equal(sc.cpu(), scores)                     # read, not written
    bar = _head_bar(scores)
    err = float((got - want).abs().max())
    print('seg_head %s: max |diff| %.3g, bar %.3g' % (case, err, bar))
    assert err <= bar
    v, _ = torch.topk(want, 2, dim=1)
    sure = (v[:, 0] - v[:, 1]) > 2 * bar
    assert sure.float().mean() > 0.9
    assert torch.equal(got.argmax(dim=1)[sure], want.argmax(dim=1)[sure])
    assert float((got.exp().sum(dim=1) - 1).abs().max()) < 1e-5


def test_seg_head_scores_against_torch_fp32():
    """the 1 x 1 seg conv of bf16 features with fp32 weights, at a channel window inside a wider ld and a pixel count that is
    no multiple of the 64-pixel tile: the inputs are exact in fp32, so the only difference to torch is the summation order"""
    from gcc_amd import ops
    g = torch.Generator().manual_seed(5)
    N, Cin, h, w, Cc = 2, 40, 7, 11, 19
    feat = torch.randn((N, Cin, h, w), generator=g).bfloat16()
    wgt, bias = torch.randn((Cc, Cin), generator=g) * 0.2, torch.randn(Cc, generator=g)
    want = torch.nn.functional.conv2d(feat.float(), wgt[:, :, None, None], bias)
    buf = ops.new_act(N, 56, h, w, DEV)
    x = ops.cslice(buf, 8, Cin)
    x.copy_(feat.to(DEV))
    scores = torch.full((N, Cc, h, w), float('nan'), dtype=torch.float32, device=DEV)
    ops.seg_head(x, wgt.to(DEV), bias.to(DEV), None, scores)
    # Cin products of magnitude <= max|w| max|x| summed in fp32 in another order: Cin ulps of the largest partial sum
    bound = Cin * float(np.spacing(np.float32(float((wgt.abs() @ feat.float().abs().amax(dim=(0, 2, 3)))[None].max()))))
    err = float((scores.cpu() - want).abs().max())
    print('seg scores: max |diff| %.3g, bound %.3g' % (err, bound))
    assert err <= bound


# ---- 4. whole nets against the reference -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def native(z):
    """(log-softmax, scores) of every fixture net through DrnSegEngine, computed once"""
    from gcc_amd.metric.drn_seg import DrnSegEngine
    out = {}
    for name in E.NETS:
        sd, x = E.fixture_net(z, name)
        eng = DrnSegEngine(sd).to(DEV)
        logp, scores = eng(x.to(DEV))
        out[name] = (logp.cpu(), scores.cpu(), eng)
    return out


@pytest.mark.parametrize('name', list(E.NETS))
def test_net_scores_within_twice_the_emulation_error(z, native, name):
    """max |native - ref| over the scores against 2 x emul_err.  Measured on an MI355X (profiles/r9_drn_native.txt): the ratio
    max |native - ref| / emul_err is 1.03 (bneck), 1.00 (basic) and 1.00 (d105thin)."""
    logp, scores, eng = native[name]
    ref = torch.from_numpy(z[name + '.scores'])
    emul = float(z[name + '.emul_err'])
    assert scores.dtype == torch.float32 and tuple(scores.shape) == tuple(ref.shape)
    N, _, H, W = (int(v) for v in z[name + '.input_shape'])
    assert logp.dtype == torch.float32 and tuple(logp.shape) == (N, 19, H, W)
    err = float((scores - ref).abs().max())
    print('%s: max |native - ref| %.4f, emul_err %.4f, ratio %.2f' % (name, err, emul, err / emul))
    assert err <= 2 * emul
    # the bilinear-like taps sum to at most ~1, so the arg-max holds wherever the reference's margin exceeds 4 emul_err
    sure = z[name + '.margin'] > 4 * emul
    assert sure.mean() > 0.25
    assert np.array_equal(logp.argmax(dim=1).numpy()[sure], z[name + '.argmax'][sure])
    # the second output is the head of the first, as in DRNSeg.forward
    sd, _ = E.fixture_net(z, name)
    assert float((logp - E.head(scores, sd['up.weight'])).abs().max()) <= _head_bar(scores)


def test_engine_repeats_itself_and_counts_its_launches(z, native):
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    L = ops.lib()
    logp, scores, eng = native['bneck']
    _, x = E.fixture_net(z, 'bneck')
    xd = x.to(DEV)
    predicted = eng.infer_launches(*[int(v) for v in (x.shape[0], x.shape[2], x.shape[3])])
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    l2, s2 = eng(xd)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(1) == predicted
    assert torch.equal(l2.cpu(), logp) and torch.equal(s2.cpu(), scores)
    # another batch size through the same engine, then the first again: the slab only grows, results do not change
    l1, s1 = eng(xd[:1].contiguous())
    assert torch.equal(s1.cpu(), scores[:1]) and torch.equal(l1.cpu(), logp[:1])
    # a fresh engine whose slab has to grow between calls: the smaller size runs again on the new slab, same bits
    from gcc_amd.metric.drn_seg import DrnSegEngine
    eng2 = DrnSegEngine(E.fixture_net(z, 'bneck')[0]).to(DEV)
    a1 = eng2(xd[:1].contiguous())[1]
    small = eng2._slab.numel()
    a2 = eng2(xd)[1]
    assert eng2._slab.numel() > small
    a3 = eng2(xd[:1].contiguous())[1]
    assert torch.equal(a1.cpu(), scores[:1]) and torch.equal(a2.cpu(), scores) and torch.equal(a3.cpu(), scores[:1])
    with pytest.raises(GccError, match='multiples of 32'):
        eng(torch.zeros(1, 3, 64, 80, device=DEV))
    with pytest.raises(GccError, match='the input is on cpu'):
        eng(x)


# ---- 5. end to end: the reference's own --drn_path file ---------------------------------------------------------------------------
ARGV = ['--model', 'pix2pix', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp', '--print_freq', '1000']


def _root(tmp_path, z):
    zm = np.load(ME.GOLDEN)
    rng = np.random.RandomState(3)
    names = [str(n) for n in zm['names']]
    photos = {n: rng.randint(0, 256, (256, 512, 3), dtype=np.uint8) for n in names}
    root = tmp_path / 'cityscapes'
    ME.write_root(str(root), zm, photos)
    drn = tmp_path / 'drn-d_fixture.pth'
    torch.save(E.fixture_net(z, 'bneck')[0], str(drn))         # a plain state_dict, as util.load_network reads it
    return root, drn


def test_cli_prints_the_miou_of_the_native_segmenter(tmp_path, z):
    from gcc_amd.metric import cityscapes as CS
    from gcc_amd.metric.drn_seg import DrnSegEngine
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    root, drn = _root(tmp_path, z)
    argv = ['--dataroot', str(root), '--drn_path', str(drn), '--checkpoints_dir', str(tmp_path / 'ck')] + ARGV
    opt = options.parse(argv)
    opt.isTrain = True
    model = get_model_class(opt)(opt)
    model.netG.load_state_dict({k: v.to(DEV) for k, v in recipe_state_dict(O.unet_shapes(8, 8), 23).items()})
    model.refresh_weights()
    model.save_models(1, str(tmp_path / 'save'))
    model.model_eval()
    seg, why = CS.builtin_segmenter(opt)
    assert isinstance(seg, DrnSegEngine) and why is None
    value = CS.cityscapes_evaluator(seg)(model, opt)[0][0]
    assert 0.0 <= value <= 100.0
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', str(tmp_path / 'save' / 'model_1.pth')],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert ('mIoU: %.2f' % value) in r.stdout.splitlines(), r.stdout[-2000:]
    assert len(list((tmp_path / 'ck' / 'exp' / 'test_results' / 'fake_B').glob('*.png'))) == 3


def test_train_logs_the_miou_and_keeps_the_best(tmp_path, z):
    from gcc_amd import train
    root, drn = _root(tmp_path, z)
    shutil.copytree(str(root / 'val'), str(root / 'train'))
    ck = tmp_path / 'ck'
    # a Cityscapes root fixes the schedule (250 epochs, an evaluation every 5): starting at 250 trains and evaluates one epoch
    model = train.main(['--dataroot', str(root), '--drn_path', str(drn), '--checkpoints_dir', str(ck), '--epoch_count', '250',
                        '--batch_size', '1'] + ARGV)
    torch.cuda.synchronize()
    log = (ck / 'exp' / 'logger.log').read_text()
    assert str(drn) in log
    values = re.findall(r'^.*mIoU: ([0-9.]+)$', log, re.M)
    assert len(values) == 1, log[-2000:]
    best = list((ck / 'exp' / 'checkpoints').glob('model_best_*.pth'))
    assert len(best) == 1 and best[0].name == 'model_best_BtoA.pth'
    assert model is not None


# ---- 6. the product's width, once -------------------------------------------------------------------------------------------------
def test_full_width_drn_d_105_once():
    from gcc_amd import ops
    from gcc_amd.metric.drn_seg import DrnSegEngine
    kind, layers, channels = E.D105
    sd = E.drn_state_dict(E.drn_shapes(kind, layers, channels), 404, damp=0.25)
    eng = DrnSegEngine(sd).to(DEV)
    del sd
    assert len(eng.convs) == 108
    x = E.seeded_input((1, 3, 256, 256), 405).to(DEV)
    L = ops.lib()
    predicted = eng.infer_launches(1, 256, 256)
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    logp, scores = eng(x)
    torch.cuda.synchronize()
    n = L.gcc_launch_count(1)
    print('drn_d_105 at 1 x 256 x 256: %d launches (predicted %d), %.1f GFLOP' % (n, predicted, eng.flops(256, 256) / 1e9))
    assert n == predicted
    assert tuple(logp.shape) == (1, 19, 256, 256) and tuple(scores.shape) == (1, 19, 32, 32)
    assert torch.isfinite(logp).all() and torch.isfinite(scores).all()
    assert float((logp.exp().sum(dim=1) - 1).abs().max()) < 1e-4
    first = scores.clone()
    slab = eng._slab.data_ptr()
    del logp, scores
    torch.cuda.synchronize()
    base, reserved = torch.cuda.memory_allocated(DEV), torch.cuda.memory_reserved(DEV)
    logp, scores = eng(x)
    torch.cuda.synchronize()
    assert torch.equal(scores, first)
    del logp, scores
    assert eng._slab.data_ptr() == slab
    assert torch.cuda.memory_allocated(DEV) == base and torch.cuda.memory_reserved(DEV) == reserved
