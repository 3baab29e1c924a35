"""--continue_train host pieces that need no GPU: the atomic state writer and the option check of a resume."""
import os

import pytest
import torch


def test_state_writer_leaves_the_previous_file_when_the_write_fails(tmp_path, monkeypatch):
    from gcc_amd import train
    path = str(tmp_path / train.STATE_FILE)
    train.write_atomic({'epoch': 1, 'w': torch.arange(4.0)}, path)
    assert torch.load(path)['epoch'] == 1

    def boom(obj, f, *a, **k):
        f.write(b'partial')
        raise RuntimeError('disk full')
    monkeypatch.setattr(torch, 'save', boom)
    with pytest.raises(RuntimeError, match='disk full'):
        train.write_atomic({'epoch': 2}, path)
    monkeypatch.undo()
    got = torch.load(path)
    assert got['epoch'] == 1 and torch.equal(got['w'], torch.arange(4.0))
    assert os.listdir(str(tmp_path)) == [train.STATE_FILE], 'the temporary file must not remain'

    train.write_atomic({'epoch': 2}, path)
    assert torch.load(path)['epoch'] == 2 and os.listdir(str(tmp_path)) == [train.STATE_FILE]


def test_resume_refuses_other_options_and_ignores_bookkeeping():
    from gcc_amd import train
    from gcc_amd._lib import GccError
    from gcc_amd.options import options
    base = ['--dataroot', 'synthetic', '--model', 'pix2pix', '--ngf', '8', '--continue_train', '1']
    stored = vars(options.parse(base))
    train.check_resume_options(dict(stored), options.parse(base + ['--print_freq', '7', '--gpu_ids', '1', '--num_threads', '2',
                                                                    '--checkpoints_dir', '/elsewhere', '--save_epoch_freq', '5']))
    with pytest.raises(GccError, match='ngf'):
        train.check_resume_options(dict(stored), options.parse(base[:-4] + ['--ngf', '16', '--continue_train', '1']))
    with pytest.raises(GccError, match=r'batch_size.*lr'):
        train.check_resume_options(dict(stored), options.parse(base + ['--lr', '1e-3', '--batch_size', '4']))


def test_continue_train_parses_as_the_reference_does():
    """type=bool, kept from the reference's option table: any non-empty value is true -- '--continue_train 1' is the spelling"""
    from gcc_amd.options import options
    assert options.parse([]).continue_train is False
    assert options.parse(['--continue_train', '1']).continue_train is True
    assert options.parse(['--continue_train', 'False']).continue_train is True
