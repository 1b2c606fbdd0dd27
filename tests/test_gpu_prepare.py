"""From Vis-MVSNet output to a scene that trains, through the three commands: tools/fusion.py -> all_torch.ply -> cut.ply ->
tools/vismvsnet2mvsdf.py -> SceneDataset / DeviceBatches / tools/train.py's runner, on the directory tests/mvs_scene.py writes."""
import importlib.util
import os
import shutil

import numpy as np
import pytest
import torch

import featext_ref
import mvs_scene as S
import train_scene
from conftest import ROOT
from mvsdf_amd import chamfer, fusion, training
from mvsdf_amd.datasets import prepare
from mvsdf_amd.datasets.device_batches import DeviceBatches
from mvsdf_amd.datasets.scene_dataset import SceneDataset
from mvsdf_amd.utils import io as sio

pytestmark = pytest.mark.gpu
PTHRESH = '.8,.7,.8'


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fused(root, **kw):
    pair, cams, depths, probs = prepare.load_mvs_output(root)
    return fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs, **kw), pair


def _box_scale_mat(points_f32):
    lo, hi = points_f32.min(0), points_f32.max(0)
    sm = np.eye(4, dtype=np.float32)
    sm[:3, :3] *= (torch.from_numpy(hi - lo).max() * 1.1).item() / 2             # the cloud's box x 1.1 (vismvsnet2mvsdf.py:86-88, 112-114)
    sm[:3, 3] = (lo + hi) / 2
    return sm


@pytest.fixture(scope='module')
def mvs(tmp_path_factory):
    root, ids = S.write_mvs_scene(tmp_path_factory.mktemp('mvs'), n_views=4, clean=True)
    ckpt = os.path.join(root, 'vismvsnet.pt')
    torch.save(featext_ref.make_checkpoint(5), ckpt)
    return root, ids, ckpt


def test_three_commands_from_mvs_output_to_a_training_run(mvs, tmp_path, capsys):
    root, ids, ckpt = mvs
    # 1. fusion
    _tool('fusion').main(['--data', root, '--pair', os.path.join(root, 'pair.txt'), '--view', '10', '--vthresh', '2', '--pthresh', PTHRESH,
                          '--no_normal', '--downsample', '-1'])
    f, pair = _fused(root)
    printed = capsys.readouterr().out
    assert 'total: %d points' % len(f) in printed and all('view %s: ' % i in printed for i in ids) and len(f) > 500
    ply = os.path.join(root, 'all_torch.ply')
    cloud = chamfer.load_points(ply)
    want = f.points.cpu().numpy().astype(np.float32)
    assert np.array_equal(cloud.astype(np.float32), want) and np.array_equal(cloud, want.astype(np.float64))
    from mvsdf_amd.mesh import _ply_elements
    small = np.stack([prepare.resize_bilinear_u8(prepare.load_image_u8(os.path.join(root, '%s.jpg' % i.zfill(8))), 28, 20) for i in ids])
    v, p = f.view.cpu().numpy(), f.pixel.cpu().numpy()
    vert = _ply_elements(ply)['vertex']
    assert np.array_equal(np.stack([vert[k] for k in ('red', 'green', 'blue')], 1), small[v, p // 28, p % 28])
    # 2. the manual cut (here: none) and the converter
    shutil.copy(ply, os.path.join(root, 'cut.ply'))
    _tool('vismvsnet2mvsdf').main(['--data_root', root, '--prob_mask', '--pthresh', PTHRESH, '--resize', '96,72', '--crop', '96,72',
                                   '--ext_image_path', os.path.join(root, '{:08}.jpg')])
    scene = os.path.join(root, 'imfunc4')
    ds = SceneDataset(scene, False, feat_ckpt=ckpt)
    assert len(ds) == 4 and tuple(ds.img_res) == (72, 96)
    assert np.array_equal(np.asarray(ds.get_scale_mat()), _box_scale_mat(want))
    assert torch.equal(ds.depths[:, 0], f.masked_depths.to(ds.depths.device))
    db = DeviceBatches(ds, 2, 100, seed=0)
    idx, mi, gt = next(iter(db))
    assert mi['uv'].shape == (2, 100, 2) and mi['uv'].is_cuda and bool(mi['object_mask'].any())
    # 3. one epoch of training on it
    conf = train_scene.write_conf(tmp_path / 'test.conf', plot_freq='1/1', milestones=('1/1',))
    lines = []
    r = training.main(['--data_dir', scene, '--conf', conf, '--batch_size', '2', '--nepoch', '1', '--expname', 'byod', '--gpu', 'ignore',
                       '--exps_root', str(tmp_path / 'exps'), '--seed', '0', '--feat_ckpt', ckpt], printer=lines.append)
    steps = [ln for ln in lines if ln.startswith('mvsdf_byod [')]
    assert len(steps) >= 2 and all(np.isfinite(float(ln.split('loss = ')[1].split(',')[0].split()[0])) for ln in steps)
    for p_ in r.model.parameters():
        assert bool(torch.isfinite(p_).all())


def test_range_source_fused_and_fused_depth(mvs, tmp_path):
    root0, ids, ckpt = mvs
    root = str(tmp_path / 'mvs')
    shutil.copytree(root0, root, ignore=shutil.ignore_patterns('imfunc4', '*.ply'))
    f, pair = _fused(root, pthresh=(0.8, 0.7, 0.8))
    tool = _tool('vismvsnet2mvsdf')
    common = ['--data_root', root, '--prob_mask', '--pthresh', PTHRESH, '--resize', '96,72', '--crop', '96,72', '--ext_image_path', os.path.join(root, '{:08}.jpg')]
    tool.main(common + ['--range_source', 'fused'])
    cloud = chamfer.load_points(os.path.join(root, 'all_torch.ply'))
    want = f.points.cpu().numpy().astype(np.float32)
    assert np.array_equal(cloud.astype(np.float32), want)
    fused_cams = dict(np.load(os.path.join(root, 'imfunc4', 'cameras_hd.npz')))
    assert np.array_equal(fused_cams['scale_mat_0'], _box_scale_mat(want))
    for i in range(4):
        assert np.array_equal(sio.load_pfm(os.path.join(root, 'imfunc4', 'depth', '%03d.pfm' % i)), f.masked_depths[i].cpu().numpy())
    shutil.copy(os.path.join(root, 'all_torch.ply'), os.path.join(root, 'cut.ply'))      # an uncut cut.ply: the same scale_mat
    tool.main(common + ['--fused_depth'])
    pcd_cams = np.load(os.path.join(root, 'imfunc4', 'cameras_hd.npz'))
    assert sorted(pcd_cams.files) == sorted(fused_cams)
    for k in fused_cams:
        assert np.array_equal(pcd_cams[k], fused_cams[k]), k
    for i in range(4):
        got = sio.load_pfm(os.path.join(root, 'imfunc4', 'depth', '%03d.pfm' % i))
        assert np.array_equal(got, f.fused_depths[i].cpu().numpy())
    assert float((f.fused_depths > 0).sum()) < float((f.masked_depths > 0).sum())
