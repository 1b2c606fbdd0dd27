"""The training and evaluation commands on the device: DeviceBatches (csrc/batch_kernels.hip) against SceneDataset items + collate_fn, the runner
against the same steps written out by hand, the run's directory tree, resume and seeding, and tools/eval.py against the pieces it is made of."""
import glob
import os
import time

import numpy as np
import pytest
import torch

from mvsdf_amd import evaluation, mesh, training
from mvsdf_amd.datasets.device_batches import DeviceBatches
from mvsdf_amd.datasets.scene_dataset import SceneDataset

import train_scene

pytestmark = pytest.mark.gpu
N_VIEWS = 4


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    return train_scene.write_scene(tmp_path_factory.mktemp('dtu'), N_VIEWS, pmask=True)


@pytest.fixture(scope='module')
def scene_nopm(tmp_path_factory):
    return train_scene.write_scene(tmp_path_factory.mktemp('dtu_nopm'), 3, pmask=False, seed=1)


@pytest.fixture(scope='module')
def conf(tmp_path_factory):
    return train_scene.write_conf(tmp_path_factory.mktemp('conf') / 'test.conf')


def _collated(ds, views, pix):
    ds.sampling_idx = None if pix is None else pix.cpu()
    try:
        return ds.collate_fn([ds[int(i)] for i in views])
    finally:
        ds.sampling_idx = None


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, (what, a.shape, b.shape, a.dtype, b.dtype, a.device, b.device)
    assert a.stride() == b.stride(), (what, a.stride(), b.stride())
    assert torch.equal(a, b), what


def _check_batch(ds, db, views, pix):
    idx, mi, gt = db.batch(torch.tensor(views), None, pix)
    ridx, rmi, rgt = _collated(ds, views, pix)
    assert torch.equal(idx, ridx) and not idx.is_cuda
    assert list(mi) == list(rmi) and list(gt) == list(rgt)
    for k in rmi:
        _same(mi[k], rmi[k].cuda() if not rmi[k].is_cuda else rmi[k], 'model_input.' + k)
    for k in rgt:
        _same(gt[k], rgt[k].cuda() if not rgt[k].is_cuda else rgt[k], 'ground_truth.' + k)
    assert gt['feat'].stride(1) == 1 and gt['feat_src'].stride(2) == 1


@pytest.mark.parametrize('pm', [True, False])
def test_device_batches_equal_collated_items(scene, scene_nopm, pm):
    d, ck = scene if pm else scene_nopm
    ds = SceneDataset(d, False, feat_ckpt=ck)
    assert hasattr(ds, 'perfect_masks') == pm
    db = DeviceBatches(ds, 2, 100, seed=0)
    g = torch.Generator(device='cuda').manual_seed(7)
    pix = torch.randperm(ds.total_pixels, device='cuda', generator=g)[:100]           # 100 pixels: not a multiple of 64
    n = len(ds)
    _check_batch(ds, db, [n - 1, 0], pix)                                                 # views out of order
    _check_batch(ds, db, [1], pix)                                                        # B = 1
    _check_batch(ds, db, [2, 0, 1][:n], None)                                             # whole images (change_sampling_idx(-1))
    _check_batch(ds, db, list(range(n))[::-1], pix[:37])
    # an epoch: drop_last view order from the host generator, pixel sample from the device generator, the batches of that order
    db = DeviceBatches(ds, 2, 100, seed=3)
    batches = list(db)
    assert len(batches) == n // 2 and db.sampling_idx.shape == (100,) and db.sampling_idx.is_cuda
    order = db.epoch_views
    assert order.shape == (n // 2 * 2,) and len(set(order.tolist())) == order.numel()
    for i, (idx, mi, gt) in enumerate(batches):
        assert torch.equal(idx, order[2 * i:2 * i + 2])
        ridx, rmi, rgt = _collated(ds, idx, db.sampling_idx)
        for k in rgt:
            assert torch.equal(gt[k], rgt[k].cuda()), k
        assert torch.equal(mi['uv'], rmi['uv'].cuda()) and torch.equal(mi['object_mask'], rmi['object_mask'].cuda())
    full = DeviceBatches(ds, 1, -1, seed=0)
    (idx, mi, gt), = list(full)[:1]
    assert full.sampling_idx is None and mi['uv'].shape == (1, ds.total_pixels, 2)


def test_device_batches_never_wait(scene):
    ds = SceneDataset(scene[0], False, feat_ckpt=scene[1])
    db = DeviceBatches(ds, 2, 100, seed=0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for _ in range(2):                                                                # two epochs: the per-epoch draws included
            for idx, mi, gt in db:
                pass
    finally:
        torch.cuda.set_sync_debug_mode('default')
    # the reference's item: its pageable host-to-device copies (scene_dataset.py:129, 137) each synchronise
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            ds[0]
    finally:
        torch.cuda.set_sync_debug_mode('default')


def test_sel_depth_num_other_than_one_is_refused(scene):
    ds = SceneDataset(scene[0], False, feat_ckpt=scene[1])
    ds.sel_depth_num = 2
    with pytest.raises(NotImplementedError):
        DeviceBatches(ds, 2, 100)


def _runner(scene, conf, root, **kw):
    args = dict(conf=conf, data_dir=scene[0], batch_size=2, nepochs=4, expname='t', gpu_index='ignore', exps_folder_name='exps', is_continue=False,
                timestamp='latest', checkpoint='latest', train_cameras=False, exps_root=str(root), seed=0, feat_ckpt=scene[1], printer=lambda *a: None)
    args.update(kw)
    return training.IDRTrainRunner(**args)


def test_runner_equals_the_loop_written_out(scene, conf, tmp_path):
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.model.loss import IDRLoss
    from mvsdf_amd.optim import FlatAdam
    r = _runner(scene, conf, tmp_path)
    sd0 = {k: v.detach().clone() for k, v in r.model.state_dict().items()}
    torch.manual_seed(11)
    draws = []
    for epoch in range(3):                                                # epoch 0: phase 0 (no cap), epoch 1: tp = 1/4 (cap 2), epoch 2: a milestone
        r.train_epoch(epoch)
        draws.append((r.batches.epoch_views.clone(), r.batches.sampling_idx.clone()))
    r.log.flush()
    # the same steps by hand: items, collate, IDRNetwork, IDRLoss, FlatAdam with the conf's grad cap, MultiStepLR
    sched_conf = training.schedule_module()
    ds = r.train_dataset
    model = IDRNetwork(r.conf.get_config('model')).cuda()
    model.load_state_dict(sd0)
    opt = FlatAdam(model.parameters(), lr=2e-4 * 2)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [2, 3], gamma=0.5)
    loss_fn = IDRLoss()
    torch.manual_seed(11)
    want = []
    for epoch, (views, pix) in enumerate(draws):
        tp = epoch / 4
        cap = sched_conf.grad_cap(tp) if sched_conf.phase[0] <= tp and sched_conf.enable_grad_cap else None
        for i in range(len(views) // 2):
            _, mi, gt = _collated(ds, views[2 * i:2 * i + 2], pix)
            mi = {k: v.cuda() for k, v in mi.items()}
            gt = {k: v.cuda() for k, v in gt.items()}
            opt.zero_grad()
            out = model(mi, tp)
            lo = loss_fn(out, gt, tp, 2)
            opt.backward(lo['loss'])
            opt.step(grad_cap=cap)
            want.append(([float(lo[k].detach().reshape(-1)[0]) for k in training.LOSS_KEYS], float(opt.grad_norm())))
        sched.step()
    for (k, a), b in zip(r.model.state_dict().items(), model.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(r.optimizer.flat_m, opt.flat_m) and torch.equal(r.optimizer.flat_v, opt.flat_v)
    assert r.optimizer._t == opt._t == 6
    assert r.scheduler.state_dict() == sched.state_dict()
    got = [(vals, gn) for _, _, vals, gn in r.log.records]
    assert [(e, i) for e, i, _, _ in r.log.records] == [(e, i) for e in range(3) for i in range(2)]
    assert got == want
    # the runner's step loop (batches, model, loss, backward, optimiser, lagged log) asks nothing of the GPU: no call synchronises
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r.train_epoch(3)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    r.log.flush()
    assert [(e, i) for e, i, _, _ in r.log.records[-2:]] == [(3, 0), (3, 1)]


def _tree(run):
    return sorted(os.path.relpath(p, run) for p in glob.glob(os.path.join(run, '**', '*'), recursive=True))


def test_run_layout_resume_and_seed(scene, conf, tmp_path):
    lines = []
    argv = ['--data_dir', scene[0], '--conf', conf, '--batch_size', '2', '--nepoch', '2', '--expname', 'run', '--gpu', 'ignore',
            '--exps_root', str(tmp_path / 'a'), '--seed', '5', '--feat_ckpt', scene[1]]
    r = training.main(argv, printer=lines.append)
    runs = os.listdir(str(tmp_path / 'a' / 'exps' / 'mvsdf_run'))
    assert runs == [r.timestamp]
    run = str(tmp_path / 'a' / 'exps' / 'mvsdf_run' / r.timestamp)
    ck = ['checkpoints/%s/%s.pth' % (s, e) for s in ('ModelParameters', 'OptimizerParameters', 'SchedulerParameters') for e in ('1', '2', 'latest')]
    want = sorted(['checkpoints', 'plots', 'checkpoints/ModelParameters', 'checkpoints/OptimizerParameters', 'checkpoints/SchedulerParameters']
                  + ck + ['plots/surface_1.obj', 'plots/surface_2.obj'])
    assert _tree(run) == want                                                   # plot_freq = 1/2 of 2 epochs: checkpoints + plots at epochs 1 and 2
    steps = [ln for ln in lines if ln.startswith('mvsdf_run [')]
    assert len(steps) == 3 * 2 and steps[0].startswith('mvsdf_run [0/2] (0/2): loss = ') and steps[-1].startswith('mvsdf_run [2/2] (1/2): ')
    assert sum(ln.startswith('grad norm: ') for ln in lines) == 6 and sum(ln.startswith('grad cap: ') for ln in lines) == 4
    # the full plot (every fourth plot epoch) on demand: rendering above ground truth, and the depth map
    r.plot_epoch(2, full=True)
    from PIL import Image
    H, W = r.img_res
    assert Image.open(os.path.join(run, 'plots', 'rendering_2.png')).size == (W + 4, 2 * (H + 2) + 2)
    assert Image.open(os.path.join(run, 'plots', 'depth_2.png')).size == (W, H)
    # --is_continue: the newest run, the latest checkpoint, a new timestamp directory
    time.sleep(1.1)
    r2 = _runner(scene, conf, tmp_path / 'a', nepochs=2, expname='run', is_continue=True, seed=None)
    assert r2.start_epoch == 2 and r2.timestamp != r.timestamp
    for (k, a), b in zip(r.model.state_dict().items(), r2.model.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(r.optimizer.flat_m, r2.optimizer.flat_m) and torch.equal(r.optimizer.flat_v, r2.optimizer.flat_v)
    assert r2.optimizer._t == r.optimizer._t and r2.optimizer.param_groups[0]['lr'] == r.optimizer.param_groups[0]['lr']
    assert r2.scheduler.state_dict() == r.scheduler.state_dict()
    # the same seed, another run: the same parameters at the end
    r3 = training.main([a if a != str(tmp_path / 'a') else str(tmp_path / 'b') for a in argv], printer=lambda *a: None)
    for (k, a), b in zip(r.model.state_dict().items(), r3.model.state_dict().values()):
        assert torch.equal(a, b), k


def test_eval_command(scene, scene_nopm, conf, tmp_path):
    root = str(tmp_path)
    r = training.main(['--data_dir', scene[0], '--conf', conf, '--batch_size', '2', '--nepoch', '2', '--expname', 'ev', '--gpu', 'ignore',
                       '--exps_root', root, '--seed', '1', '--feat_ckpt', scene[1]], printer=lambda *a: None)
    out = []
    res = evaluation.main(['--data_dir', scene[0], '--conf', conf, '--expname', 'ev', '--exps_root', root, '--feat_ckpt', scene[1],
                           '--resolution', '48', '--eval_rendering'], printer=out.append)
    evaldir = os.path.join(root, 'evals', 'mvsdf_ev')
    assert res['evaldir'] == evaldir and res['epoch'] == 2
    got = mesh.load_mesh(os.path.join(evaldir, 'surface_world_coordinates_2.obj'))
    ds = r.train_dataset
    ref = evaluation.extract_world_mesh(r.model, ds.get_scale_mat(), 48)
    assert torch.equal(got.vertices.cpu().float(), ref.vertices.cpu().float()) and torch.equal(got.faces.cpu().long(), ref.faces.cpu().long())
    pngs = sorted(os.listdir(os.path.join(evaldir, 'rendering')))
    assert pngs == ['eval_%03d.png' % i for i in range(N_VIEWS)]
    db = DeviceBatches(ds, 1, -1)
    batches = []
    for i in range(N_VIEWS):
        _, mi, gt = db.batch(torch.tensor([i]))
        mi['object_mask'] = mi['perfect_mask']
        batches.append((mi, gt))
    psnrs, _ = evaluation.evaluate_rendering(r.model, batches, ds.img_res)
    line = open(os.path.join(evaldir, 'psnr.txt')).read()
    assert line == 'RENDERING EVALUATION mvsdf_ev: psnr mean = %.2f ; psnr std = %.2f\n' % (np.mean(psnrs), np.std(psnrs))
    assert out[-1] == line.strip()
    # a scene without pmask/: a clear error
    with pytest.raises(ValueError, match='pmask'):
        evaluation.main(['--data_dir', scene_nopm[0], '--conf', conf, '--expname', 'ev', '--exps_root', root, '--feat_ckpt', scene_nopm[1],
                         '--resolution', '16', '--eval_rendering'], printer=lambda *a: None)
