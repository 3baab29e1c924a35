"""python -m gcc_amd.metric.get_real_stat: the reference's metric/get_real_stat.py -- the Inception statistics (mu, sigma) of a
dataset's real images, the real_stat*.npz a FID evaluation compares against.

    python -m gcc_amd.metric.get_real_stat --dataroot ./database/edges2shoes --direction AtoB \\
        --output_path ./database/edges2shoes/real_stat_B.npz
    python -m gcc_amd.metric.get_real_stat --dataroot ./database/celeb --dataset_mode sa --crop_size 64 --center_crop \\
        --output_path ./database/celeb/real_stat.npz

The reference's arguments and defaults; ``--dataset_mode unaligned`` is accepted as well (domain B for AtoB, A for BtoA), so
that CycleGAN roots get theirs.  The network is the file GCC_FID_INCEPTION names: the reference's weight file or a TorchScript archive (gcc_amd.metric.fid_eval).
The weight file runs natively at the precision GCC_FID_PRECISION names (bf16, the default, or fp32: the reference's own); the tool
prints which one wrote the file.  Write the real statistics through the same route as the scores compared against them.
Images are read through gcc_amd.data, keyed by path (a repeated path counts once), turned into the network's input by
gcc_fid_input -- util.tensor2imgs' byte of the loader's [-1, 1] tensor over 255, exactly: 63 of the 256 byte values come back
one lower from that round trip, and the reference's statistics are statistics of those bytes -- and go through the network at
batch 32 (the reference's value) into the streamed statistics.  The file is the reference's: np.savez(mu=, sigma=) in f64.
``--features_path F.npz`` (this tool's own flag) also writes the activations those statistics were built from,
np.savez(act=<fp32 [n, d]>, network=<which network made them>): named real_act*.npz beside its real_stat*.npz, it lets every FID
evaluation report the Kernel Inception Distance as well (gcc_amd.metric.kid_score).

``--dims 64|192|768|2048`` (this tool's own flag too; unset: GCC_FID_DIMS, else 2048) writes the statistics -- and the activations
-- of the reference's narrower output blocks: what a FID evaluation under the same GCC_FID_DIMS, or fid_score --dims, compares
against.

One difference: the reference sets max_dataset_size = -1, which makes its file listing drop whichever file os.walk listed
last; this tool reads every file of the split."""
import argparse
import warnings

import numpy as np
import torch

from .._lib import GccError

BATCH_SIZE = 32              # metric/get_real_stat.py:32

parser = argparse.ArgumentParser(description='Extract some statistical information of a dataset to compute FID')
parser.add_argument('--input_nc', type=int, default=3)
parser.add_argument('--output_nc', type=int, default=3)
parser.add_argument('--dataroot', required=True, help='path to images (should have subfolders trainA, trainB, valA, valB, train, val, etc)')
parser.add_argument('--dataset_mode', type=str, default='aligned', help='[aligned | sa | unaligned]')
parser.add_argument('--direction', type=str, default='AtoB', help='AtoB or BtoA')
parser.add_argument('--load_size', type=int, default=256, help='scale images to this size')
parser.add_argument('--crop_size', type=int, default=256, help='then crop to this size')
parser.add_argument('--preprocess', type=str, default='none',
                    help='[resize_and_crop | crop | scale_width | scale_width_and_crop | none]')
parser.add_argument('--phase', type=str, default='val', help='train, val, test, etc')
parser.add_argument('--output_path', type=str, required=True, help='the path to save the statistical information.')
parser.add_argument('--gpu_ids', type=str, default='0', help='gpu ids: the first one is used')
parser.add_argument('--z_dim', type=int, default=128)
parser.add_argument('--center_crop', action='store_true')
# `parser` is the reference's surface, argument for argument; the tool parses with it plus the flags that are its own
tool_parser = argparse.ArgumentParser(parents=[parser], add_help=False, description=parser.description)
tool_parser.add_argument('--features_path', type=str, default=None,
                         help='also save the activations the statistics were built from (np.savez(act=, network=)): a '
                              'real_act*.npz beside its real_stat*.npz lets every FID evaluation report KID as well')

# ... and the width, on a parser of its own around the two: the flags of `parser` and `tool_parser` stay what they were
dims_parser = argparse.ArgumentParser(parents=[tool_parser], add_help=False, description=parser.description)
dims_parser.add_argument('--dims', type=int, default=None, choices=[64, 192, 768, 2048],
                         help='width of the features: the output block the native network is tapped at (unset: GCC_FID_DIMS, '
                              'else 2048); a TorchScript archive runs as exported')

# dataset mode -> (image, its path) of a batch, per direction
_PICK = {'aligned': lambda AtoB: ('B', 'B_paths') if AtoB else ('A', 'A_paths'),
         'unaligned': lambda AtoB: ('B', 'B_paths') if AtoB else ('A', 'A_paths'),
         'sa': lambda AtoB: ('real_img', 'img_path')}


def parse(argv=None):
    opt = dims_parser.parse_args(argv)
    if opt.dataset_mode not in _PICK:
        raise GccError('get_real_stat: --dataset_mode %s (aligned, sa and unaligned have real images to score)' % opt.dataset_mode)
    opt.num_threads, opt.batch_size, opt.serial_batches, opt.no_flip = 0, 1, True, True
    opt.max_dataset_size = float('inf')
    opt.gpu_ids = [i for i in (int(s) for s in str(opt.gpu_ids).split(',')) if i >= 0]
    from .fid_eval import fid_dims
    opt.dims = fid_dims(opt.dims)
    return opt


def real_statistics(opt, inception, device, batch_size=BATCH_SIZE, features=False):
    """(mu [d], sigma [d, d]) f64 device tensors of the split's real images; ``features``: and the fp32 [n, d] activations they
    were built from, as a third element"""
    from ..data import create_dataset
    from .cityscapes import _prepare, adopt_batch
    from .fid_eval import ImageStatistics
    image, path = _PICK[opt.dataset_mode](opt.direction == 'AtoB')
    stats = ImageStatistics(_prepare(inception, device), batch_size, keep_features=features)
    cur = torch.cuda.current_stream(device)
    for data in create_dataset(opt, device):
        adopt_batch(data, cur)
        stats.add(data[path][0], data[image])
    return stats.result() + ((stats.features.rows(),) if features else ())


def main(argv=None, inception=None):
    opt = parse(argv)
    if not opt.output_path.endswith('.npz'):
        warnings.warn('The output is a numpy npz file, but the output path does\'nt end with ".npz".')
    if not torch.cuda.is_available() or not opt.gpu_ids:
        raise GccError('gcc_amd runs on MI355X only (no CPU path): need a visible GPU')
    if len(opt.gpu_ids) > 1:
        warnings.warn('The code only supports single GPU. Only gpu [%d] will be used.' % opt.gpu_ids[0])
    torch.cuda.set_device(opt.gpu_ids[0])
    device = torch.device('cuda', opt.gpu_ids[0])
    if inception is None:
        from .fid_eval import load_inception
        inception, why = load_inception(opt.dims)
        if inception is None:
            raise GccError('get_real_stat: %s' % why)
    mu, sigma, *act = real_statistics(opt, inception, device, features=opt.features_path is not None)
    np.savez(opt.output_path, mu=mu.cpu().numpy(), sigma=sigma.cpu().numpy())
    from .fid_eval import network_label
    if act:
        from .kid_score import save_features
        save_features(opt.features_path, act[0], network_label(inception))
        print('get_real_stat: %s written (%d x %d activations)' % ((opt.features_path,) + tuple(act[0].shape)))
    print('get_real_stat: %s written with the Inception network%s' % (opt.output_path, network_label(inception) or ' (TorchScript)'))
    return opt.output_path


if __name__ == '__main__':
    main()
