"""Steady-state ms per training step of three loops on one synthetic DTU-sized scene (49 views of 1600 x 1200, depth maps and features of 600 x 800,
written by tests/train_scene.py), at the c2 shape (W = 256, 8 views x 256 px) and the shipped shape (W = 512, 8 views x 4096 px):

  (a) runner     mvsdf_amd.training.IDRTrainRunner.train_epoch: DeviceBatches (one gather launch per step), lagged log lines
  (b) prebuilt   the same zero_grad / model / IDRLoss / backward / FlatAdam loop on batches assembled in advance (bench.py's protocol, no log)
  (c) reference  SceneDataset + DataLoader(shuffle, drop_last) + change_sampling_idx + .cuda() + the reference's per-step .item() prints

Every loop runs whole epochs at train_progress 0.3 (phase 1, like bench.py) after one warm-up epoch, with frozen weights (lr = 0, like bench.py), and all
three run the same steps: (b) and (c) replay the view orders and pixel samples (a) drew.  No plot or checkpoint epoch is timed.  (a) and (b) alternate
--reps times and the medians are reported; host_enqueue_ms_per_step is the host's own loop time (the deferred step lets it run ahead).  --gather: the batch gather alone against a device-to-device copy of the same feature bytes, under
HIP events (run it behind `rocprofv3 --kernel-trace --memory-copy-trace --stats` for the kernel's own duration).  Prints one JSON line per shape."""
import argparse
import gc
import io
import json
import os
import sys
import tempfile
import time
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_scene  # noqa: E402
from mvsdf_amd import training  # noqa: E402

SHAPES = {'c2': (256, 256), 'shipped': (512, 4096)}          # name: (W, pixels per view)
TP_EPOCH, NEPOCHS = 3, 10                                    # train_progress = 3 / 10 = 0.3 for every timed epoch


def runner_for(scene, root, W, P, batch):
    conf = train_scene.write_conf(os.path.join(root, 'time_%d_%d.conf' % (W, P)), W=W, num_pixels=P, plot_freq='1/1', resolution=32)
    sink = io.StringIO()
    r = training.IDRTrainRunner(conf=conf, data_dir=scene[0], batch_size=batch, nepochs=NEPOCHS, expname='time', gpu_index='ignore',
                                exps_folder_name='exps', is_continue=False, timestamp='latest', checkpoint='latest', train_cameras=False,
                                exps_root=root, seed=0, feat_ckpt=scene[1], printer=lambda *a: sink.write(' '.join(map(str, a)) + '\n'))
    return r


HOST_MS = {}


def timed(fn, steps, key=None):
    """-> wall ms per step; the host's enqueue time per step (fn's own duration: the deferred step lets the host run ahead) goes to HOST_MS[key]."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    if key is not None:
        HOST_MS.setdefault(key, []).append((t1 - t0) / steps * 1e3)
    return (time.perf_counter() - t0) / steps * 1e3


def loop_runner(r, epochs, draws=None):
    def run():
        for _ in range(epochs):
            r.train_epoch(TP_EPOCH)
            if draws is not None:
                draws.append((r.batches.epoch_views.clone(), r.batches.sampling_idx.clone()))
    return run


def loop_prebuilt(r, epochs_of_batches):
    tp = TP_EPOCH / NEPOCHS
    sched = training.schedule_module()
    cap = sched.grad_cap(tp) if sched.phase[0] <= tp and sched.enable_grad_cap else None

    def run():
        for batches in epochs_of_batches:
            for _, mi, gt in batches:
                r.optimizer.zero_grad()
                out = r.model(mi, tp)
                lo = r.loss(out, dict(gt), tp, r.n_batches)
                r.optimizer.backward(lo['loss'])
                r.optimizer.step(grad_cap=cap, zero_grad=True)
    return run


class _Order(torch.utils.data.Sampler):
    """The batch sampler of loop (c): the view order loop (a) drew, epoch by epoch (the content of the steps equal across the loops)."""

    def __init__(self, draws, B):
        self.draws, self.B, self.k = draws, B, 0

    def __iter__(self):
        views = self.draws[self.k % len(self.draws)][0].tolist()
        self.k += 1
        return iter([views[i:i + self.B] for i in range(0, len(views), self.B)])

    def __len__(self):
        return len(self.draws[0][0]) // self.B


def loop_reference(r, draws, printer):
    ds = r.train_dataset
    order = _Order(draws, r.batch_size)
    dl = torch.utils.data.DataLoader(ds, batch_sampler=order, collate_fn=ds.collate_fn)
    tp = TP_EPOCH / NEPOCHS
    sched = training.schedule_module()
    cap = sched.grad_cap(tp) if sched.phase[0] <= tp and sched.enable_grad_cap else None
    pix = [d[1].cpu() for d in draws]

    def run():
        for e in range(len(draws)):
            ds.change_sampling_idx(r.num_pixels)                               # the reference's per-epoch CPU randperm (its cost) ...
            ds.sampling_idx = pix[e]                                           # ... and loop (a)'s pixel sample (its content)
            for data_index, (indices, mi, gt) in enumerate(dl):
                for k in ('intrinsics', 'uv', 'object_mask', 'pose'):
                    mi[k] = mi[k].cuda()
                r.optimizer.zero_grad()
                out = r.model(mi, tp)
                lo = r.loss(out, gt, tp, len(dl))
                r.optimizer.backward(lo['loss'])
                printer('grad norm:', r.optimizer.grad_norm().item())          # idr_train.py:289-313: seven .item() per step
                r.optimizer.step(grad_cap=cap, zero_grad=True)
                printer(f"loss = {lo['loss'].item():.4f},", f"rgb_loss = {lo['rgb_loss'].item():.4f},", f"eikonal_loss = {lo['eikonal_loss'].item():.4f},",
                        f"feat_loss = {lo['feat_loss'].item():.4f},", f"depth_loss = {lo['depth_loss'].item():.4f},", f"surf_loss = {lo['surf_loss'].item():.4f}")
        ds.change_sampling_idx(-1)
    return run


def time_shape(scene, root, name, epochs, reps, batch):
    """Every loop runs the SAME steps: frozen weights (lr = 0, like bench.py), and (b) / (c) replay the view orders and pixel samples (a) drew."""
    W, P = SHAPES[name]
    r = runner_for(scene, root, W, P, batch)
    r.optimizer.param_groups[0]['lr'] = 0.0
    steps = epochs * r.n_batches
    db = r.batches
    out = {'a': [], 'b': [], 'c': []}
    HOST_MS.clear()
    loop_runner(r, 1)()                                          # warm-up epoch (the step plans, the allocator's blocks)
    states = (db.gen_host.get_state(), db.gen_dev.get_state())

    def rewind():
        db.gen_host.set_state(states[0])
        db.gen_dev.set_state(states[1])
    draws = []
    rewind()
    loop_runner(r, epochs, draws)()
    rewind()
    pre = [list(db) for _ in range(epochs)]                      # (b)'s batches: the same draws, assembled before the clock starts
    loop_prebuilt(r, pre[:1])()
    for _ in range(reps):
        rewind()
        out['a'].append(timed(loop_runner(r, epochs), steps, 'a'))
        r.log.flush()
        out['b'].append(timed(loop_prebuilt(r, pre), steps, 'b'))
    del pre
    sink = io.StringIO()
    with redirect_stdout(sink):
        p = lambda *a: print(*a)
        loop_reference(r, draws[:1], p)()
        out['c'].append(timed(loop_reference(r, draws, p), steps, 'c'))
    med = {k: float(np.median(v)) for k, v in out.items()}
    host = {k: float(np.median(v)) for k, v in HOST_MS.items()}
    return {'shape': name, 'W': W, 'views': r.batch_size, 'px_per_view': P, 'steps_per_epoch': r.n_batches, 'timed_steps': steps, 'reps': reps,
            'ms_per_step': {'a_runner': med['a'], 'b_prebuilt': med['b'], 'c_reference_loop': med['c']},
            'host_enqueue_ms_per_step': host, 'runs_ms': out, 'a_over_b': med['a'] / med['b'], 'c_over_b': med['c'] / med['b']}


def time_gather(scene, iters):
    from mvsdf_amd.datasets.device_batches import DeviceBatches
    from mvsdf_amd.datasets.scene_dataset import SceneDataset
    ds = SceneDataset(scene[0], False, feat_ckpt=scene[1])
    res = {}
    for name, P in (('c2', 256), ('shipped', 4096)):
        db = DeviceBatches(ds, 8, P, seed=0)
        db.new_epoch()
        views = db.epoch_views[:8]
        vd = db._views_dev[:8]
        fbytes = 8 * (1 + db.num_src) * db.feats[0].numel() * 4
        other = 8 * P * (12 + 8 + 1 + (1 if db.pmask is not None else 0)) + 8 * db.depths[0].numel() * 4 + 8 * (100 + 32 * db.num_src) * 4
        src = torch.empty(fbytes // 4, device='cuda')
        dst = torch.empty_like(src)
        for _ in range(3):
            db.batch(views, vd, db.sampling_idx)
            dst.copy_(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        for _ in range(iters):
            db.batch(views, vd, db.sampling_idx)
        ev[1].record()
        for _ in range(iters):
            dst.copy_(src)
        ev[2].record()
        torch.cuda.synchronize()
        tg = ev[0].elapsed_time(ev[1]) / iters * 1e3
        tc = ev[1].elapsed_time(ev[2]) / iters * 1e3
        moved = 2 * (fbytes + other)
        res[name] = {'gather_us': tg, 'feature_bytes': fbytes, 'bytes_moved': moved, 'gather_bytes_per_us': moved / tg,
                     'dtod_copy_us': tc, 'dtod_bytes_per_us': 2 * fbytes / tc}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c2,shipped')
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--epochs', type=int, default=4, help='timed epochs per run')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gather', action='store_true')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        t0 = time.time()
        scene = train_scene.write_scene(root, a.views, pmask=True, img_wh=(1600, 1200), depth_hw=(600, 800))
        sys.stderr.write('scene written in %.1f s\n' % (time.time() - t0))
        results = []
        if a.gather:
            results.append({'gather': time_gather(scene, a.iters)})
        else:
            for name in a.shapes.split(','):
                results.append(time_shape(scene, root, name, a.epochs, a.reps, 8))
                gc.collect()
                torch.cuda.empty_cache()
        for res in results:
            print(json.dumps(res))
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
