"""The training / evaluation commands' host logic (mvsdf_amd/training.py, evaluation.py): configuration parsing, the exps tree, argument defaults, the
reference's log lines and the numpy make_grid.  No GPU."""
import os

import numpy as np

from mvsdf_amd import evaluation, training
from mvsdf_amd.utils.config import load_conf, parse_hocon

import train_scene


def test_milestones_and_plot_freq_follow_the_reference(tmp_path):
    conf = parse_hocon('train{\n expname = mvsdf\n plot_freq = 1/12\n sched_milestones = [4/6,5/6]\n sched_factor = 0.1\n}\n')
    assert training.fraction('1/12') == 1 / 12
    assert training.sched_milestones(conf, 1800) == [1200, 1500]
    assert training.sched_milestones(conf, 7) == [int(7 * (4 / 6)), int(7 * (5 / 6))] == [4, 5]
    assert training.sched_factor(conf) == 0.1
    assert training.plot_freq(conf, 1800) == 150
    assert training.plot_freq(conf, 13) == 1
    bare = parse_hocon('train{\n plot_freq = 1/2\n}\n')
    assert training.sched_milestones(bare, 100) == [] and training.sched_factor(bare) == 0.0
    c = load_conf(train_scene.write_conf(tmp_path / 'x.conf'))
    assert training.plot_freq(c, 4) == 2 and training.sched_milestones(c, 4) == [2, 3]
    assert c.get_config('model').get_config('implicit_network')['dims'] == [64] * 8
    assert c.get_string('train.expname') == 'mvsdf' and c.get_int('plot.resolution') == 32


def test_latest_timestamp_and_continue(tmp_path):
    expdir = str(tmp_path / 'exps' / 'mvsdf_a')
    assert training.latest_timestamp(expdir) is None
    assert training.resolve_continue(expdir, True, 'latest') == (False, None)       # nothing to continue from
    os.makedirs(expdir)
    assert training.resolve_continue(expdir, True, 'latest') == (False, None)
    for ts in ('2024_01_02_10_00_00', '2024_11_02_09_00_00', '2024_03_02_23_59_59'):
        os.makedirs(os.path.join(expdir, ts))
    assert training.latest_timestamp(expdir) == '2024_11_02_09_00_00'
    assert training.resolve_continue(expdir, True, 'latest') == (True, '2024_11_02_09_00_00')
    assert training.resolve_continue(expdir, True, '2024_01_02_10_00_00') == (True, '2024_01_02_10_00_00')
    assert training.resolve_continue(expdir, False, 'latest') == (False, 'latest')   # the reference passes these through untouched


def test_argument_defaults():
    a = training.parser().parse_args([])
    assert (a.data_dir, a.batch_size, a.nepoch, a.conf, a.expname, a.gpu) == ('fill_in_data_dir', 8, 1800, './confs/mvsdf_dtu.conf', 'test', 'auto')
    assert (a.is_continue, a.timestamp, a.checkpoint) == (False, 'latest', 'latest')
    assert (a.exps_root, a.seed, a.feat_ckpt) == ('../', None, None)
    a = training.parser().parse_args(['--is_continue', '--seed', '3', '--batch_size', '2', '--exps_root', '/x'])
    assert a.is_continue and a.seed == 3 and a.batch_size == 2 and a.exps_root == '/x'
    e = evaluation.eval_parser().parse_args([])
    assert (e.data_dir, e.conf, e.expname, e.exps_folder, e.timestamp, e.checkpoint, e.resolution, e.eval_rendering) == \
        ('fill_in_data_dir', './confs/mvsdf_dtu.conf', 'test', 'exps', 'latest', 'latest', 512, False)
    assert (e.exps_root, e.feat_ckpt) == ('../', None)


def test_log_lines_from_scalars():
    vals = [1.23456, 0.5, 0.01234, 0.0, 2.00005, 0.1]
    lines = training.step_lines('mvsdf_scan', 3, 1800, 1, 6, vals, np.float32(0.75), 2, 0.0016)
    assert lines == ['grad norm: 0.75', 'grad cap: 2',
                     'mvsdf_scan [3/1800] (1/6): loss = 1.2346, rgb_loss = 0.5000, eikonal_loss = 0.0123, feat_loss = 0.0000, '
                     'depth_loss = 2.0000, surf_loss = 0.1000, lr = 0.0016']
    # before phase[0] there is no cap line; the grad norm prints as the float it is (float32 -> Python float, like .item())
    lines = training.step_lines('e', 0, 10, 0, 1, vals, np.float32(0.1), None, 0.0002)
    assert len(lines) == 2 and lines[0] == 'grad norm: %s' % float(np.float32(0.1)) and lines[1].endswith('lr = 0.0002')


def test_make_grid_is_torchvisions():
    rs = np.random.RandomState(0)
    two = rs.uniform(size=(2, 3, 4, 5)).astype(np.float32)
    g = training.make_grid(two, nrow=1)
    assert g.shape == (3, 2 * (4 + 2) + 2, 5 + 4)
    assert np.array_equal(g[:, 2:6, 2:7], two[0]) and np.array_equal(g[:, 8:12, 2:7], two[1])
    assert g[:, :2].max() == 0 and g[:, 6:8].max() == 0 and g[:, :, :2].max() == 0
    one = rs.uniform(1, 5, size=(1, 1, 4, 5)).astype(np.float32)
    n = training.make_grid(one, nrow=1, normalize=True, scale_each=True)     # a single image comes back without padding, normalised to [0, 1]
    assert n.shape == (3, 4, 5) and n.min() == 0 and abs(n.max() - 1) < 1e-6
    assert np.allclose(n[0], (one[0, 0] - one.min()) / (one.max() - one.min()))



def test_batch_args_mirror_matches_the_library():
    import ctypes
    from mvsdf_amd import _lib
    from mvsdf_amd.datasets.device_batches import BatchArgs
    assert _lib.lib().mvsdf_batch_args_bytes() == ctypes.sizeof(BatchArgs)
