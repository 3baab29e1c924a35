"""python -m gcc_amd.test: the reference's test.py (test.py:12-130) -- load a (pruned) checkpoint with its cfg, run the generator
over the test split, write PNGs under <checkpoints_dir>/<name>/test_results with the names of the reference's util.save_images.

Same flags as gcc_amd.train (--pretrain_path is required).  Per model:
  pix2pix   phase val, batch 1, serial, no flip, load_size 256; the generator through Pix2PixModel.infer_nhwc (fused eval path)
            at the precision GCC_GEN_PRECISION names (bf16, the default, or fp32: the reference's own; U-Net only);
            --backbone resnet and cyclegan: MobileResnetEngine.infer at the precision GCC_RESNET_PRECISION names;
            on a Cityscapes root with table.txt and a segmenter at --drn_path (the reference's .pth or TorchScript): prints the mIoU afterwards
  pix2pix (other roots), cyclegan, sagan: with a TorchScript Inception network at GCC_FID_INCEPTION and real_stat*.npz under
            --dataroot, prints the FID of the images written (cyclegan: also of generator B's, which are not written), and
            their KID on the next line when a real_act*.npz (get_real_stat --features_path) lies beside every real_stat*.npz,
            and with GCC_FID_PRDC=<k> their precision / recall / density / coverage on one more; with GCC_FID_IS=<splits> and
            the native network's weight file their Inception Score (IS: mean +- std over the splits) on the last
  srgan     every test/{Set5, Set14, B100, Urban100} present; the generator through SRResNetEngine.infer, at the precision
            GCC_SR_PRECISION names (bf16, the default, or fp32: the reference's own)
  cyclegan  phase test, visual_forward, visuals real_A / fake_B
  sagan     the first 1000 batches; the generator through SAGANModel.infer_nhwc (fused eval path)
Generated images are converted to bytes on the device (gcc_image_to_u8: the reference's tensor2im) and copied to the host once
per batch; input images (fp32) go through the same arithmetic on the host.  PNGs are encoded by PIL on host threads."""
import copy
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

RESULT_LABELS_REAL = ('real_A', 'real_img')
RESULT_LABELS_FAKE = ('fake_B', 'fake_A', 'fake_hr', 'fake_img')
SR_TEST_SETS = ('Set5', 'Set14', 'B100', 'Urban100')


# ---- plain host helpers (no GPU) -------------------------------------------------------------------------------------------
def _stem(path):
    return (path.split('/')[-1].split('\\')[-1]).split('.')[0]


def result_names(labels, img_path, direction='AtoB'):
    """[(label, path relative to the result directory)] of the visuals util.save_images writes (utils/util.py:208-230):
    real_A / real_img -> <imageB_name>.png; fakes -> <label>/<imageA_name>_<label>.png (fake_A: imageB_name).  img_path is
    model.image_paths ([A paths, B paths] as set_input orders them); other labels are not written."""
    first = lambda p: p[0] if isinstance(p, (list, tuple)) else p
    a_path = first(img_path[0]) if direction == 'AtoB' else first(img_path[1])
    b_path = first(img_path[1]) if direction == 'AtoB' else first(img_path[0])
    a_name, b_name = _stem(a_path), _stem(b_path)
    out = []
    for label in labels:
        if label in RESULT_LABELS_REAL:
            out.append((label, b_name + '.png'))
        if label in RESULT_LABELS_FAKE:
            out.append((label, os.path.join(label, '%s_%s.png' % (b_name if label == 'fake_A' else a_name, label))))
    return out


def test_overrides(opt):
    """the per-model option overrides of the reference's test functions (test.py:12-111) on a copy of opt; srgan's phase is
    set per test set"""
    opt = copy.deepcopy(opt)
    opt.batch_size = 1
    opt.serial_batches = True
    if opt.model == 'pix2pix':
        opt.phase, opt.num_threads, opt.no_flip, opt.load_size = 'val', 0, True, 256
    elif opt.model == 'cyclegan':
        opt.phase, opt.num_threads, opt.no_flip, opt.load_size = 'test', 0, True, 256
    elif opt.model == 'sagan':
        opt.num_threads, opt.load_size = 0, 64
    return opt


def model_kwargs(model, cfg):
    """constructor keywords of a model rebuilt from a checkpoint's 'cfg' entry"""
    pair = tuple(cfg) if isinstance(cfg, (list, tuple)) and len(cfg) == 2 else (cfg, None)
    if model == 'cyclegan':
        return {'cfg_AtoB': pair[0], 'cfg_BtoA': pair[1]}
    if model == 'pix2pix':
        return {'filter_cfgs': pair[0], 'channel_cfgs': pair[1]}
    return {'filter_cfgs': pair[0]}


def tensor2im_host(x):
    """the reference's util.tensor2im of image 0 of an NCHW fp32 tensor, on the host"""
    a = x[0].detach().float().cpu().numpy()
    return ((np.transpose(a, (1, 2, 0)) + np.float32(1)) / np.float32(2.0) * np.float32(255.0)).astype(np.uint8)


def save_image(image, path, aspect_ratio=1.0):
    """utils/util.py save_image: PIL, BICUBIC resize for an aspect ratio != 1"""
    from PIL import Image
    im = Image.fromarray(image)
    h, w, _ = image.shape
    if aspect_ratio > 1.0:
        im = im.resize((h, int(w * aspect_ratio)), Image.BICUBIC)
    if aspect_ratio < 1.0:
        im = im.resize((int(h / aspect_ratio), w), Image.BICUBIC)
    im.save(path)


# ---- the run -------------------------------------------------------------------------------------------------------------
class _Writer:
    """PNG encoding on host threads; the pixels of generated images arrive as uint8 from the device"""

    def __init__(self, result_dir, direction, aspect_ratio):
        self.dir, self.direction, self.aspect = result_dir, direction, aspect_ratio
        self.pool = ThreadPoolExecutor(max_workers=4)
        self.pending = []

    def write(self, visuals, img_path):
        """visuals: label -> NHWC device view, bf16 or fp32, or its uint8 [N, H, W, 3] bytes (generated), or NCHW fp32 tensor
        (input)"""
        from . import ops
        names = result_names(list(visuals), img_path, self.direction)
        # generated: NHWC bf16, or an NHWC fp32 view (channels innermost in a pixel stride of a multiple of 4: ops.geom_f32)
        generated = lambda t: t.dtype in (torch.bfloat16, torch.uint8) or (t.dtype == torch.float32 and t.is_cuda and t.stride(1) == 1
                                                                          and t.stride(3) % 4 == 0)
        u8 = lambda t: t if t.dtype == torch.uint8 else ops.image_to_u8(t)
        dev = [u8(visuals[label])[0] for label, _ in names if generated(visuals[label])]
        host = iter(torch.stack(dev).cpu().numpy() if dev else [])        # one device-to-host copy per batch
        for label, rel in names:
            im = next(host) if generated(visuals[label]) else tensor2im_host(visuals[label])
            path = os.path.join(self.dir, rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            # the reference passes `aspect_ratio==aspect_ratio` (True == 1.0) for the input image: only fakes are resized
            aspect = 1.0 if label in RESULT_LABELS_REAL else self.aspect
            self.pending.append(self.pool.submit(save_image, im, path, aspect))

    def close(self):
        for f in self.pending:
            f.result()
        self.pool.shutdown()


def _nhwc(x):
    """NHWC bf16 device copy of an NCHW fp32 image batch (a visual the model keeps as fp32)"""
    from . import ops
    if x.dtype == torch.bfloat16:
        return x
    N, _, H, W = x.shape
    return ops.nchw_to_nhwc(x.to(torch.float32).contiguous(), ops.new_act(N, 3, H, W, x.device))


def run(opt, model):
    from .data import create_dataset
    result_dir = os.path.join(opt.checkpoints_dir, opt.name, 'test_results')
    os.makedirs(result_dir, exist_ok=True)
    topt = test_overrides(opt)
    model.model_eval()
    if opt.model == 'srgan':
        G = model.G
        for set_name in SR_TEST_SETS:
            if not os.path.isdir(os.path.join(str(opt.dataroot), 'test', set_name)):
                continue
            sopt = copy.deepcopy(topt)
            sopt.phase = 'test/' + set_name
            w = _Writer(os.path.join(result_dir, set_name), opt.direction, opt.aspect_ratio)
            from .metric.sr_eval import infer_image, sr_precision
            precision = sr_precision()
            G.eval_coeffs(precision)
            for data in create_dataset(sopt, model.device):
                model.set_input(data)
                lr = data['lr'].to(model.device, torch.float32).contiguous()
                w.write({'fake_hr': infer_image(G, lr, precision)}, model.image_paths)
            w.close()
        return result_dir
    w = _Writer(result_dir, opt.direction, opt.aspect_ratio)
    scorer = None
    if opt.model == 'pix2pix' and 'cityscapes' in str(opt.dataroot):      # metric/test_metric.py:78-87 on the images written here
        from .metric.cityscapes import builtin_segmenter, cityscapes_evaluator
        segmenter, why = builtin_segmenter(opt)
        if segmenter is None:
            print('no Cityscapes evaluation: %s' % why)
        else:
            scorer = cityscapes_evaluator(segmenter).scorer(model, topt)
    fid = None
    from .metric import fid_eval
    if fid_eval.wants_fid(opt):                  # metric/test_metric.py:15-45, 129-204 on the images written here
        inception, why = fid_eval.builtin_inception(opt)
        if inception is None:
            print('no FID evaluation: %s' % why)
        else:
            fid = fid_eval.fid_evaluator(inception).scorer(model, topt)
    if opt.model == 'pix2pix':
        from .models.Pix2Pix import gen_precision, resnet_precision
        precision = gen_precision(only_bf16='--backbone resnet' if model.resnet else None)
        print('generator precision: %s' % (resnet_precision() if model.resnet else precision))
    elif opt.model == 'cyclegan':
        from .models.Pix2Pix import resnet_precision
        if resnet_precision() != 'bf16':         # the default run's lines stay as they were
            print('generator precision: %s' % resnet_precision())
    elif opt.model == 'sagan':
        from .models.SAGAN import sagan_precision
        if sagan_precision() != 'bf16':          # the default run's lines stay as they were
            print('generator precision: %s' % sagan_precision())
    dataset = create_dataset(topt, model.device)
    if scorer is not None and getattr(dataset, 'paths', None) is not None:
        scorer.prefetch(dataset.paths)
    for i, data in enumerate(dataset):
        if opt.model == 'sagan' and i == 1000:
            break
        model.set_input(data)
        if opt.model == 'pix2pix':
            fake = model.infer_nhwc(model.real_A)
            if fake.dtype == torch.float32:      # the fp32 route: tensor2im's bytes once, for the PNG and both scorers
                from . import ops
                fake = ops.image_to_u8(fake)
            visuals = {'real_A': model.real_A, 'fake_B': fake}
            if scorer is not None:
                scorer.add(data['A_paths'][0], visuals['fake_B'])
            if fid is not None:
                fid.add(data['A_paths'][0], visuals['fake_B'])
        elif opt.model == 'cyclegan':
            visuals = {'real_A': model.real_A, 'fake_B': model.infer_nhwc(model.real_A, 'A')}
            if fid is not None:                  # the second generator runs for its score only
                fid.add(data['A_paths'][0], visuals['fake_B'], 0)
                fid.add(data['B_paths'][0], model.infer_nhwc(model.real_B, 'B'), 1)
        elif opt.model == 'sagan':
            fake = model.infer_nhwc(data)
            if fake.dtype == torch.float32:      # the fp32 route: tensor2im's bytes once, for the PNG and the scorer
                from . import ops
                fake = ops.image_to_u8(fake)
            visuals = {'fake_img': fake, 'real_img': model.real_img}
            if fid is not None:
                fid.add(data['img_path'][0], visuals['fake_img'])
        else:
            with torch.no_grad():
                model.forward()
            v = model.get_current_visuals()
            visuals = {k: (_nhwc(t) if k in RESULT_LABELS_FAKE else t) for k, t in v.items()}
        w.write(visuals, model.image_paths)
    w.close()
    if scorer is not None:
        print('mIoU: %.2f' % scorer.result())
    if fid is not None:
        print(fid_eval.fid_line(fid.result(), fid.tags, opt.model))
        kid = fid.kid()                          # a real_act*.npz beside every real_stat*.npz: the KID of the same images
        if kid is not None:
            print(fid_eval.kid_line(kid, fid.tags, opt.model))
        prdc = fid.prdc()                        # GCC_FID_PRDC=<k>: precision / recall / density / coverage of the same images
        if prdc is not None:
            print(fid_eval.prdc_line(prdc, fid.tags, opt.model))
        score = fid.inception_score()            # GCC_FID_IS=<splits>: the Inception Score of the same images
        if score is not None:
            print(fid_eval.is_line(score, fid.tags, opt.model))
    return result_dir


def main(argv=None):
    from .models import get_model_class
    from .options import options
    opt = options.parse(argv)
    opt.isTrain = True
    os.makedirs(os.path.join(opt.checkpoints_dir, opt.name), exist_ok=True)
    if not opt.pretrain_path or not os.path.exists(opt.pretrain_path):
        raise FileNotFoundError('pretrain model path must be exist!!!')
    ckpt = torch.load(opt.pretrain_path, map_location='cpu', weights_only=False)
    model = get_model_class(opt)(opt, **model_kwargs(opt.model, ckpt.get('cfg')))
    model.load_models(opt.pretrain_path, load_discriminator=False)
    return run(opt, model)


if __name__ == '__main__':
    main()
