"""SRGAN's fp32 inference route (SRResNetEngine.infer(x, 'fp32'): one gcc_conv_eval_f32_act launch per convolution) against a
float64 restatement of the generator (tests/_srresnet_f64.py): on the reference-written checkpoint, whose own fp32 image is the
error unit, and on seeded nets whose image fills [-1, 1]; its launch count, memory and repeatability; the bf16 route beside it;
the evaluator and the two command-line tools under GCC_SR_PRECISION=fp32."""
import copy
import re

import numpy as np
import pytest
import torch

from tests import _srresnet_f64 as S
from tests.test_sr_infer_gpu import _infer as _infer_bf16
from tests.test_sr_infer_gpu import _lr, _srgan, _write_pngs
from tests.test_sr_infer_gpu import test_generator_infer_launch_count as bf16_launch_bound

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
MARGIN = 8                       # native against float64, in units of an fp32 torch evaluation's distance from float64
PRUNED = [13, 24, 64, 8, 40, 64, 17, 32, 64, 48, 9, 64, 56, 64, 16, 24]
NETS = {'ngf64': (64, None, (1, 17, 23)), 'pruned': (64, PRUNED, (1, 9, 11)), 'ngf16': (16, None, (2, 6, 7))}


def _infer_fp32(model, lr, coeffs=True):
    from gcc_amd import ops
    G = model.G
    if coeffs:
        G.eval_coeffs('fp32')
    N, _, h, w = lr.shape
    x = ops.nchw_to_nhwc_f32(lr.to(DEV).contiguous(), G.infer_input(N, h, w, 'fp32'))
    out = G.infer(x, 'fp32')
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, 3, 4 * h, 4 * w) and out.stride(1) == 1
    return ops.nhwc_to_nchw_f32(out).cpu()


def _load(model, sd):
    model.netG.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    model.refresh_weights()
    model.model_eval()
    return model


@pytest.fixture(scope='module')
def nets():
    """name -> (model, lr, float64 image, fp32 torch image on the host) of the seeded range-filling nets, computed once"""
    out = {}
    for i, (name, (ngf, cfgs, (N, h, w))) in enumerate(NETS.items()):
        model, _ = _srgan(ngf, cfgs, seed=31 + i)
        lr = _lr(N, h, w, seed=h * w)
        sd = S.fill_range({k: v.cpu() for k, v in model.netG.state_dict().items()}, lr, seed=41 + i)
        _load(model, sd)
        with torch.no_grad():
            out[name] = (model, lr, S.forward(sd, lr), S.forward(sd, lr, dtype=torch.float32))
    return out


# ---- the reference's checkpoint ------------------------------------------------------------------------------------------------
def test_reference_checkpoint_within_eight_times_the_references_own_error():
    """max |fake_hr - f64| <= 2e-8 holds the helper to the fixture; then max |native - f64| <= 8 max |fake_hr - f64|, the bar of the
    fp32 DRN-D and Inception tests on the same kernel (the summation order differs from torch's).  The bf16 route on the same
    input is more than 100 x the reference's own error away: the test can tell the routes apart.
    Measured on an MI355X (profiles/r13_sr_fp32.txt): 1.56e-8 against the reference's 1.33e-8, ratio 1.18; the bf16 route 1.44e-4."""
    sd, lr, fake_hr = S.load_fixture()
    with torch.no_grad():
        f64 = S.forward(sd, lr)
    ref_err = float((fake_hr.double() - f64).abs().max())
    assert ref_err <= 2e-8, ref_err
    model = _load(_srgan(8)[0], sd)
    got = _infer_fp32(model, lr)
    err = float((got.double() - f64).abs().max())
    bf16_err = float((_infer_bf16(model, lr).double() - f64).abs().max())
    print('reference checkpoint: max |native - f64| %.3g, max |fake_hr - f64| %.3g, ratio %.2f; bf16 route %.3g (%.0f x)'
          % (err, ref_err, err / ref_err, bf16_err, bf16_err / ref_err))
    assert err <= MARGIN * ref_err
    assert bf16_err > 100 * ref_err


# ---- seeded nets that fill the range ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(NETS))
def test_range_filling_net_within_eight_times_an_fp32_restatement(nets, name):
    """max |native - f64| <= 8 max |fp32 torch restatement - f64|, the restatement evaluated where the float64 one is (the host:
    the same text in fp32).  The image must fill the range without saturating tanh, or small errors would hide in its flat ends.
    Measured on an MI355X (profiles/r13_sr_fp32.txt): ratios 1.98 (ngf64: 3.50e-6 against 1.77e-6), 2.04 (pruned: 3.72e-6 against
    1.83e-6) and 1.02 (ngf16: 1.57e-6 against 1.54e-6); the bf16 route 1.2e-2 to 1.5e-2."""
    model, lr, f64, f32 = nets[name]
    assert S.fills_range(f64), (float(f64.std()), float((f64.abs() > 0.99).double().mean()))
    yard = float((f32.double() - f64).abs().max())
    got = _infer_fp32(model, lr)
    err = float((got.double() - f64).abs().max())
    bf16_err = float((_infer_bf16(model, lr).double() - f64).abs().max())
    print('%s: image std %.3f, max |native - f64| %.3g, max |fp32 torch - f64| %.3g, ratio %.2f; bf16 route %.3g'
          % (name, float(f64.std()), err, yard, err / yard, bf16_err))
    assert yard > 0 and err <= MARGIN * yard
    assert bf16_err > 100 * yard


# ---- launches, memory, repeatability -----------------------------------------------------------------------------------------------
def test_one_launch_per_convolution_and_no_allocation_in_the_second_eval_coeffs(nets):
    from gcc_amd import ops
    model = nets['ngf16'][0]
    G, L = model.G, ops.lib()
    n_convs = sum(1 for m in model.netG.modules() if isinstance(m, torch.nn.Conv2d))
    assert n_convs == 37
    G.eval_coeffs('fp32')
    for N, h, w in ((1, 17, 23), (2, 6, 7)):
        x = ops.nchw_to_nhwc_f32(_lr(N, h, w, 3).to(DEV).contiguous(), G.infer_input(N, h, w, 'fp32'))
        torch.cuda.synchronize()
        L.gcc_launch_count(1)
        G.infer(x, 'fp32')
        assert L.gcc_launch_count(1) == n_convs
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    G.eval_coeffs('fp32')
    G.eval_coeffs('fp32')
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base


def test_memory_is_flat_across_sizes(nets):
    model = nets['ngf16'][0]
    sizes = [(128, 128), (120, 90), (96, 96), (85, 128), (72, 72), (70, 70), (64, 64), (57, 86), (32, 48), (17, 23), (9, 11),
             (6, 7)]                                  # the size list of tests/test_sr_infer_gpu.py
    ctx0, bufs0 = set(model.G.ctx), set(model._bufs)
    _infer_fp32(model, _lr(1, *sizes[0], seed=1))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for i, (h, w) in enumerate(sizes[1:]):
        _infer_fp32(model, _lr(1, h, w, seed=i + 2))
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() - base <= 1 << 20, ((h, w), torch.cuda.memory_allocated() - base)
    assert set(model.G.ctx) == ctx0 and set(model._bufs) == bufs0


def test_repeatable_and_batch_independent(nets):
    model, lr, _, _ = nets['ngf16']
    a = _infer_fp32(model, lr)
    b = _infer_fp32(model, lr)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    one = _infer_fp32(model, lr[:1])
    assert torch.equal(one.view(torch.int32), a[:1].contiguous().view(torch.int32))


def test_the_bf16_route_is_untouched_beside_it(nets):
    from gcc_amd import _lib, ops
    model, lr, _, _ = nets['pruned']
    L = ops.lib()

    def bf16():
        G = model.G
        G.eval_coeffs()
        N, _, h, w = lr.shape
        x = ops.nchw_to_nhwc(lr.to(DEV).contiguous(), G.infer_input(N, h, w), cfill=8)
        torch.cuda.synchronize()
        L.gcc_launch_count(1)
        out = G.infer(x)
        n = L.gcc_launch_count(1)
        return ops.nhwc_to_nchw(out, 3).cpu(), n
    before, n0 = bf16()
    _infer_fp32(model, lr)
    after, n1 = bf16()
    assert torch.equal(before.view(torch.int32), after.view(torch.int32)) and n0 == n1
    bf16_launch_bound()                              # the bf16 test's own bound, in a process that has run the fp32 route
    with pytest.raises(_lib.GccError, match="eval_coeffs\\('fp32'\\)"):
        fresh, _ = _srgan(8)
        fresh.G.infer(fresh.G.infer_input(1, 6, 7, 'fp32'), 'fp32')
    for call in (lambda: model.G.infer(None, 'fp16'), lambda: model.G.eval_coeffs('fp16'), lambda: model.G.infer_input(1, 6, 7, 'fp16')):
        with pytest.raises(_lib.GccError, match='fp16'):
            call()


# ---- the evaluator ------------------------------------------------------------------------------------------------------------
def test_evaluator_follows_the_variable(tmp_path, monkeypatch):
    from gcc_amd import _lib, metric
    from gcc_amd.data import create_dataset
    from oracle import metric_oracle as M
    _write_pngs(tmp_path / 'test' / 'Set5', [(68, 92), (72, 88)], 3)             # LR 17 x 23 and 18 x 22
    model, opt = _srgan(16)
    opt.dataroot = str(tmp_path)
    monkeypatch.delenv('GCC_SR_PRECISION', raising=False)
    psnr_bf16, _ = metric.test_srgan_psnr(model, opt, 'Set5')
    monkeypatch.setenv('GCC_SR_PRECISION', 'fp32')
    psnr, ssim = metric.test_srgan_psnr(model, opt, 'Set5')
    eopt = copy.deepcopy(opt)
    eopt.phase, eopt.batch_size, eopt.serial_batches = 'test/Set5', 1, True
    ps, ss = [], []
    for batch in create_dataset(eopt, DEV):
        torch.cuda.current_stream().wait_event(batch['ready'])
        fake = _infer_fp32(model, batch['lr'].float()).numpy()
        real = batch['hr'].float().cpu().numpy()
        ps.append(M.psnr_y(fake, real))
        ss.append(M.ssim_y(fake, real))
    assert len(ps) == 2
    print('PSNR fp32 %.6f (oracle on its images %.6f), bf16 %.6f; SSIM fp32 %.8f' % (psnr, float(np.mean(ps)), psnr_bf16, ssim))
    assert abs(psnr - float(np.mean(ps))) <= 1e-3, (psnr, np.mean(ps))
    assert abs(ssim - float(np.mean(ss))) <= 1e-6, (ssim, np.mean(ss))
    assert psnr != psnr_bf16
    monkeypatch.setenv('GCC_SR_PRECISION', 'fp64')
    with pytest.raises(_lib.GccError, match='GCC_SR_PRECISION=fp64'):
        metric.test_srgan_psnr(model, opt, 'Set5')


# ---- the command-line tools ---------------------------------------------------------------------------------------------------
def test_cli_train_logs_the_precision(tmp_path, monkeypatch):
    from gcc_amd import train
    from gcc_amd.options import options
    monkeypatch.setenv('GCC_VGG19_RANDOM', '1')
    monkeypatch.setenv('GCC_SR_PRECISION', 'fp32')
    _write_pngs(tmp_path / 'data' / 'train', [(48, 48)] * 2, 1)
    _write_pngs(tmp_path / 'data' / 'test' / 'Set5', [(36, 44), (28, 33)], 2)
    argv = ['--dataroot', str(tmp_path / 'data'), '--checkpoints_dir', str(tmp_path / 'ck'), '--model', 'srgan', '--ngf', '8',
            '--ndf', '8', '--image_size', '32', '--batch_size', '2', '--n_epochs', '1', '--save_epoch_freq', '1', '--gpu_ids', '0',
            '--print_freq', '1000', '--name', 'e']
    model = train.main(argv)
    torch.cuda.synchronize()
    del model
    log = (tmp_path / 'ck' / 'e' / 'logger.log').read_text()
    assert re.search(r'SRGAN evaluation every 1 epochs \(native, fp32\) on: Set5', log), log
    assert len(re.findall(r'Set5:PSNR: [0-9.]+\| SSIM: [0-9.]+', log)) == options.parse(argv).n_epochs     # one per epoch


def test_cli_test_writes_the_fp32_image(tmp_path, monkeypatch):
    from PIL import Image
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.options import options
    monkeypatch.setenv('GCC_VGG19_RANDOM', '1')
    monkeypatch.setenv('GCC_SR_PRECISION', 'fp32')
    _write_pngs(tmp_path / 'data' / 'test' / 'Set5', [(36, 44), (28, 33)], 2)
    model, _ = _srgan(8)
    sd = S.fill_range({k: v.cpu() for k, v in model.netG.state_dict().items()}, _lr(1, 9, 11, 5), seed=9)
    _load(model, sd)
    model.save_models(5, str(tmp_path), fid=7.25)
    argv = ['--dataroot', str(tmp_path / 'data'), '--checkpoints_dir', str(tmp_path / 'ck'), '--model', 'srgan', '--ngf', '8',
            '--ndf', '8', '--gpu_ids', '0', '--name', 't', '--pretrain_path', str(tmp_path / 'model_5.pth')]
    result_dir = gtest.main(argv)
    opt = gtest.test_overrides(options.parse(argv))
    opt.phase = 'test/Set5'
    seen = 0
    for data in create_dataset(opt, DEV):
        torch.cuda.current_stream().wait_event(data['ready'])
        want = gtest.tensor2im_host(_infer_fp32(model, data['lr'].float()))
        other = gtest.tensor2im_host(_infer_bf16(model, data['lr'].float().cpu()))
        model.set_input(data)
        (_, rel), = gtest.result_names(['fake_hr'], model.image_paths)
        got = np.asarray(Image.open('%s/Set5/%s' % (result_dir, rel)))
        assert got.shape == want.shape and np.array_equal(got, want)
        seen += int((want != other).any())
    assert seen > 0                                 # somewhere the bf16 route's bytes differ: the files are the fp32 route's
