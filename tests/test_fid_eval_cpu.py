"""The host side of the per-epoch FID evaluation (gcc_amd.metric.fid_eval, gcc_amd.metric.get_real_stat): where the network
comes from and why not, which real statistics a model reads, SAGAN's count rule, the tool's arguments, and the refusals that need
no device."""
import numpy as np
import pytest
import torch

from gcc_amd._lib import GccError
from gcc_amd.metric import fid_eval as E
from gcc_amd.metric import get_real_stat as G
from gcc_amd.options import options


class _Tiny(torch.nn.Module):
    def forward(self, x):
        return [x.mean((2, 3), keepdim=True)]


def _opt(model, root, *more):
    return options.parse(['--dataroot', str(root), '--model', model] + list(more))


def test_builtin_inception_names_the_four_refusals(tmp_path, monkeypatch):
    opt = _opt('pix2pix', tmp_path)
    monkeypatch.delenv(E.ENV, raising=False)
    net, why = E.builtin_inception(opt)
    assert net is None and 'GCC_FID_INCEPTION is not set' in why
    monkeypatch.setenv(E.ENV, str(tmp_path / 'absent.pt'))
    net, why = E.builtin_inception(opt)
    assert net is None and 'absent.pt does not exist' in why
    plain = tmp_path / 'state_dict.pth'
    torch.save({'w': torch.zeros(2)}, str(plain))
    monkeypatch.setenv(E.ENV, str(plain))
    net, why = E.builtin_inception(opt)
    assert net is None and 'TorchScript archive' in why and 'torch.jit' in why and '\n' not in why
    good = tmp_path / 'tiny.pt'
    torch.jit.script(_Tiny()).save(str(good))
    monkeypatch.setenv(E.ENV, str(good))
    net, why = E.builtin_inception(opt)
    assert net is None and 'holds no real_stat_B.npz' in why
    np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(3), sigma=np.eye(3))
    net, why = E.builtin_inception(opt)
    assert why is None and net(torch.zeros(2, 3, 4, 4))[0].shape == (2, 3, 1, 1)
    # cyclegan needs both files and names the missing one
    net, why = E.builtin_inception(_opt('cyclegan', tmp_path))
    assert net is None and 'real_stat_A.npz' in why and 'real_stat_B.npz' not in why


def test_builtin_evaluator_logs_the_reason_once(tmp_path, monkeypatch):
    from gcc_amd import train
    monkeypatch.delenv(E.ENV, raising=False)
    for model in ('pix2pix', 'cyclegan', 'sagan'):
        lines = []
        logger = type('L', (), {'info': staticmethod(lines.append)})
        assert train.builtin_evaluator(_opt(model, tmp_path), logger) is None
        assert lines == ['no FID evaluation: GCC_FID_INCEPTION is not set (the path of a TorchScript archive of the Inception network)']


def test_real_statistics_per_model_and_direction(tmp_path):
    assert E.real_stat_slots(_opt('pix2pix', tmp_path)) == [('real_stat_B.npz', 'AtoB')]
    assert E.real_stat_slots(_opt('pix2pix', tmp_path, '--direction', 'BtoA')) == [('real_stat_A.npz', 'BtoA')]
    assert E.real_stat_slots(_opt('pix2pix', tmp_path / 'maps')) == [('real_stat_A.npz', 'BtoA')]        # the root sets BtoA
    both = [('real_stat_B.npz', 'AtoB'), ('real_stat_A.npz', 'BtoA')]
    assert E.real_stat_slots(_opt('cyclegan', tmp_path)) == both
    assert E.real_stat_slots(_opt('cyclegan', tmp_path, '--direction', 'BtoA')) == both
    assert E.real_stat_slots(_opt('sagan', tmp_path)) == [('real_stat.npz', 'AtoB')]
    assert E.wants_fid(_opt('pix2pix', tmp_path)) and E.wants_fid(_opt('cyclegan', tmp_path)) and E.wants_fid(_opt('sagan', tmp_path))
    assert not E.wants_fid(_opt('pix2pix', tmp_path / 'cityscapes')) and not E.wants_fid(_opt('srgan', tmp_path))


@pytest.mark.parametrize('length,scored', [(9, 1), (10, 2), (20, 3), (25, 3)])
def test_sagan_count_rule(length, scored):
    """metric/test_metric.py:142-145: `if i > len(dataset) * 0.1: break` before batch i is scored"""
    got = 0
    for i in range(length):
        if i > length * 0.1:
            break
        got += 1
    assert got == scored == length // 10 + 1
    assert E.sagan_count(length) == scored
    assert [E.sagan_stops(i, length) for i in range(scored + 1)] == [False] * scored + [True]


def test_get_real_stat_arguments_are_the_reference_s():
    # metric/get_real_stat.py:38-56 (name, default; None: required) and :59-63
    reference = {'input_nc': 3, 'output_nc': 3, 'dataroot': None, 'dataset_mode': 'aligned', 'direction': 'AtoB', 'load_size': 256,
                 'crop_size': 256, 'preprocess': 'none', 'phase': 'val', 'output_path': None, 'gpu_ids': '0', 'z_dim': 128,
                 'center_crop': False}
    actions = {a.dest: a for a in G.parser._actions if a.dest != 'help'}
    assert set(actions) == set(reference)
    for name, default in reference.items():
        assert actions[name].required == (default is None), name
        if default is not None:
            assert actions[name].default == default and type(actions[name].default) is type(default), name
    opt = G.parse(['--dataroot', 'r', '--output_path', 'o.npz'])
    assert (opt.num_threads, opt.batch_size, opt.serial_batches, opt.no_flip, opt.gpu_ids) == (0, 1, True, True, [0])
    assert G.BATCH_SIZE == 32
    assert G.parse(['--dataroot', 'r', '--output_path', 'o.npz', '--dataset_mode', 'unaligned']).dataset_mode == 'unaligned'
    with pytest.raises(GccError, match='dataset_mode sr'):
        G.parse(['--dataroot', 'r', '--output_path', 'o.npz', '--dataset_mode', 'sr'])
    assert G._PICK['aligned'](True) == ('B', 'B_paths') and G._PICK['aligned'](False) == ('A', 'A_paths')
    assert G._PICK['unaligned'](True) == ('B', 'B_paths') and G._PICK['unaligned'](False) == ('A', 'A_paths')
    assert G._PICK['sa'](True) == ('real_img', 'img_path')


def test_evaluator_refuses_other_widths_and_too_few_images(tmp_path):
    np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(5), sigma=np.eye(5))
    with pytest.raises(GccError, match=r'mu \(5,\) and sigma \(5, 5\).*d = 65'):
        E.load_real_stat(str(tmp_path / 'real_stat_B.npz'), 65, 'cpu')
    np.savez(str(tmp_path / 'real_stat_A.npz'), mu=np.zeros(65), sigma=np.eye(5))
    with pytest.raises(GccError, match='d = 65'):
        E.load_real_stat(str(tmp_path / 'real_stat_A.npz'), 65, 'cpu')
    mu, sigma = E.load_real_stat(str(tmp_path / 'real_stat_B.npz'), 5, 'cpu')
    assert mu.dtype == sigma.dtype == torch.float64 and tuple(sigma.shape) == (5, 5)
    sc = E.FidScorer(_Tiny(), tmp_path, E.real_stat_slots(_opt('pix2pix', tmp_path)), batch_size=4)
    with pytest.raises(GccError, match='at least 2 images, 0 were scored'):
        sc.result()
    st = E.ImageStatistics(_Tiny(), 4)
    st.seen.add('only')                       # one image: refused before anything is flushed
    with pytest.raises(GccError, match='at least 2 images, 1 were scored'):
        st.result()
