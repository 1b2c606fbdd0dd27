"""SceneDataset (mvsdf_amd/datasets/scene_dataset.py) on a tiny synthetic scene written under tmp_path in the reference's layout: item keys,
shapes and dtypes, sources from pair.txt, device-resident channels-last features equal to extract_features, and one training step through
IDRNetwork + IDRLoss on a collated batch."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import featext_ref as R
from mvsdf_amd.datasets.scene_dataset import SceneDataset
from mvsdf_amd.features import extract_features
from mvsdf_amd.utils import io as sio
from mvsdf_amd.utils import synth

pytestmark = pytest.mark.gpu
N_VIEWS, IMG_WH, DEPTH_HW = 3, (96, 72), (20, 28)
IDS = ['4', '9', '17']                       # view i has id IDS[i] in pair.txt (cam file cam_<8-digit id>_flow3.txt)
PAIRS = {'4': ['17', '9'], '9': ['4', '17'], '17': ['9', '4']}


def _write_cam(path, cam):
    txt = 'extrinsic\n' + '\n'.join(' '.join('%.10g' % v for v in r) for r in cam[0]) + '\n\nintrinsic\n'
    txt += '\n'.join(' '.join('%.10g' % v for v in r) for r in cam[1][:3, :3]) + '\n\n425.0 2.5 192 905.0\n'
    open(path, 'w').write(txt)


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp('dtu')
    d = root / 'scan1'
    for sub in ('image_hd', 'mask_hd', 'depth'):
        (d / sub).mkdir(parents=True)
    rs = np.random.RandomState(0)
    size, center = 2.0, np.array([0.1, -0.2, 0.05])
    cams = {}
    for i in range(N_VIEWS):
        pose, K, cam = synth._camera(0.4 + 0.3 * i, 2.5, 0.8, size, center, IMG_WH, 2.2 * IMG_WH[0], DEPTH_HW)
        scale = np.eye(4)
        scale[:3, :3] *= size / 2
        scale[:3, 3] = center
        Rn = pose[:3, :3].T
        Pn = np.eye(4)
        Pn[:3, :4] = K[:3, :3] @ np.hstack([Rn, -Rn @ pose[:3, 3:4]])
        cams['world_mat_%d' % i] = Pn @ np.linalg.inv(scale)
        cams['scale_mat_%d' % i] = scale
        img = rs.randint(0, 256, (IMG_WH[1], IMG_WH[0], 3)).astype(np.uint8)
        Image.fromarray(img).save(str(d / 'image_hd' / ('%06d.png' % i)))
        mask = np.zeros((IMG_WH[1], IMG_WH[0]), np.uint8)
        mask[10:60, 20:80] = 255
        Image.fromarray(np.stack([mask] * 3, -1)).save(str(d / 'mask_hd' / ('%03d.png' % i)))
        sio.write_pfm(str(d / 'depth' / ('%03d.pfm' % i)), rs.uniform(400, 900, DEPTH_HW).astype(np.float32))
        _write_cam(str(root / ('cam_%08d_flow3.txt' % int(IDS[i]))), cam)
    np.savez(str(d / 'cameras_hd.npz'), **cams)
    with open(str(root / 'pair.txt'), 'w') as f:
        f.write('%d\n' % N_VIEWS)
        for i in IDS:
            f.write('%s\n%d %s\n' % (i, len(PAIRS[i]), ' '.join('%s %.1f' % (s, 100.0 - j) for j, s in enumerate(PAIRS[i]))))
    torch.save(R.make_checkpoint(5), str(root / 'vismvsnet.pt'))
    return str(d), str(root / 'vismvsnet.pt')


@pytest.fixture(scope='module')
def ds(scene):
    return SceneDataset(scene[0], False, feat_ckpt=scene[1])


def test_items(ds, scene):
    assert len(ds) == N_VIEWS and ds.img_res == (IMG_WH[1], IMG_WH[0])
    assert ds.feat_ext._ws is None                      # the extraction workspace is not held for the dataset's lifetime
    assert ds.rgb_2xd.shape == (N_VIEWS, 3, 2 * DEPTH_HW[0], 2 * DEPTH_HW[1])
    np.random.seed(0)
    idx, s, gt = ds[1]
    P = IMG_WH[0] * IMG_WH[1]
    assert idx == 1
    assert s['uv'].shape == (P, 2) and s['uv'].dtype == torch.float32
    assert s['object_mask'].shape == (P,) and s['object_mask'].dtype == torch.bool and s['object_mask'].sum() == 50 * 60
    assert s['intrinsics'].shape == (4, 4) and s['pose'].shape == (4, 4)
    assert gt['rgb'].shape == (P, 3) and float(gt['rgb'].abs().max()) <= 1.0
    assert gt['depths'].shape == (1, 1) + DEPTH_HW and gt['depths'].is_cuda
    assert gt['depth_cams'].shape == (1, 2, 4, 4) and gt['cam'].shape == (2, 4, 4) and gt['src_cams'].shape == (2, 2, 4, 4)
    assert gt['size'].shape == () and gt['center'].shape == (3,)
    assert gt['feat'].shape == (32,) + DEPTH_HW and gt['feat_src'].shape == (2, 32) + DEPTH_HW
    assert gt['feat'].is_cuda and gt['feat'].stride(0) == 1 and gt['feat_src'].stride(1) == 1
    for k in ('depths', 'depth_cams', 'size', 'center', 'cam', 'src_cams'):
        assert s[k] is gt[k]
    # sources follow pair.txt: view 1 = id '9' -> ids '4', '17' = views 0, 2
    assert torch.equal(gt['feat_src'][0], ds.feats[0]) and torch.equal(gt['feat_src'][1], ds.feats[2])
    assert torch.equal(gt['src_cams'], ds.cams_hd[[0, 2]])
    want = sio.scale_camera(torch.from_numpy(sio.load_cam(os.path.join(os.path.dirname(scene[0]), 'cam_00000009_flow3.txt'), 256, 1)).float(), 2)
    assert torch.equal(gt['cam'].cpu(), want)
    ds.change_sampling_idx(100)
    _, s2, gt2 = ds[0]
    assert s2['uv'].shape == (100, 2) and gt2['rgb'].shape == (100, 3) and s2['object_mask'].shape == (100,)
    ds.change_sampling_idx(-1)
    assert np.array_equal(ds.get_scale_mat(), np.load(os.path.join(scene[0], 'cameras_hd.npz'))['scale_mat_0'])


def test_cameras_decompose_back(ds, scene):
    cams = np.load(os.path.join(scene[0], 'cameras_hd.npz'))
    for i in range(N_VIEWS):
        P = (cams['world_mat_%d' % i] @ cams['scale_mat_%d' % i])[:3]
        K, pose = ds.intrinsics_all[i].double().numpy(), ds.pose_all[i].double().numpy()
        Rn = pose[:3, :3].T
        Pr = K[:3, :3] @ np.hstack([Rn, -Rn @ pose[:3, 3:4]])
        assert np.allclose(Pr / Pr[2, 3], P / P[2, 3], rtol=1e-4, atol=1e-4)


def test_features_are_extract_features(ds):
    f = extract_features(ds.feat_ext, ds.rgb_2xd)
    assert ds.feats.is_cuda and ds.feats.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(ds.feats, f)
    for i in range(N_VIEWS):
        assert torch.equal(ds[i][2]['feat'], f[i])
    # FeatExt's element [2] as the reference computes it (fp64 restatement, the same weights)
    ref = R.featext64(R.make_state_dict(5), ds.rgb_2xd)[2]
    scale = float(ref.abs().max())
    assert float((f.double().cpu() - ref).abs().max()) <= 1e-4 * scale


def test_collated_batch_trains(ds):
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.model.loss import IDRLoss
    from mvsdf_amd.utils.config import ConfigDict
    torch.manual_seed(0)
    np.random.seed(0)
    ds.change_sampling_idx(256)
    idx, s, gt = ds.collate_fn([ds[0], ds[2]])
    ds.change_sampling_idx(-1)
    assert torch.equal(idx, torch.tensor([0, 2]))
    assert gt['feat'].shape == (2, 32) + DEPTH_HW and gt['feat'].stride(1) == 1
    assert gt['feat_src'].shape == (2, 2, 32) + DEPTH_HW and gt['feat_src'].stride(2) == 1
    W = 64
    model = IDRNetwork(ConfigDict(synth.model_conf(W)))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    model = model.cuda().train()
    inp = {k: v.cuda() for k, v in s.items()}
    gtc = {k: v.cuda() for k, v in gt.items()}
    out = model(inp, 0.3)
    lo = IDRLoss()(out, gtc, 0.3, 2)
    lo['loss'].backward()
    for k in ('loss', 'rgb_loss', 'eikonal_loss', 'feat_loss', 'surf_loss'):
        if k in lo:
            assert torch.isfinite(lo[k]).all(), k
    g = torch.cat([p.grad.flatten() for p in model.parameters() if p.grad is not None])
    assert torch.isfinite(g).all() and float(g.norm()) > 0


def test_switched_off_branches(scene, monkeypatch):
    with pytest.raises(NotImplementedError):
        SceneDataset(scene[0], True, feat_ckpt=scene[1])
    monkeypatch.setenv('IDR_USE_ENV', '1')
    monkeypatch.setenv('IDR_ONLY_CAM', '1')
    with pytest.raises(NotImplementedError):
        SceneDataset(scene[0], False, feat_ckpt=scene[1])
