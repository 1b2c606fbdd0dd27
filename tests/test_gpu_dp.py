"""Data-parallel step on real device tensors: two ranks (two processes sharing the one GPU of the test box, gloo transport) each take one
view of a two-view batch; after FlatAdam.all_reduce_mean their gradient equals the single-process gradient on the whole batch
(rays shard by view, ONE all-reduce on the flat gradient buffer; the count-normalised loss terms use global counts)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED, TP = 3, 0.3
# (W, B, P, V): a small case, and the per-rank shape of BASELINE configs[3] (c4: 8x256 networks, ONE view of 2048 px per rank, 4 source
# views, depth maps replicated) with the two ranks this box can hold instead of eight
# 'c4x8' is BASELINE configs[3]'s batch itself: 8 views x 2048 px = 16384 rays, run as FOUR ranks (two views each) sharing the one GPU of the test box --
# with the pytest process that is five processes holding the GPU; a shared GPU admits at most six at a time, eight ranks would make nine
CFGS = {'small': (64, 2, 96, 2), 'c4': (256, 2, 2048, 4), 'c4x8': (256, 8, 2048, 4)}

WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, 'tests'))
from test_gpu_dp import run_step
rank, world, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
dist.init_process_group('gloo', init_method='tcp://127.0.0.1:' + sys.argv[4], rank=rank, world_size=world)
flat, losses = run_step(rank, world, sys.argv[5])
torch.save({{'flat': flat, 'losses': losses}}, out)
dist.destroy_process_group()
'''


def run_step(rank, world, cfg='small'):
    """One forward + loss + backward (+ the gradient all-reduce when a process group exists) on this rank's share of the fixed batch."""
    W, B, P, V = CFGS[cfg]
    from helpers import t
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.model.loss import IDRLoss
    from mvsdf_amd.optim import FlatAdam
    from mvsdf_amd.parallel import shard_views
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, SEED).items()})
    m = m.cuda().train()
    opt = FlatAdam(m.parameters(), lr=0.0)
    inp, gt = synth.make_batch(B, P, V, seed=SEED, feat_hw=(60, 80), size=2.3, center=(0.05, -0.1, 0.1))
    inp, gt = {k: t(v) for k, v in inp.items()}, {k: t(v) for k, v in gt.items()}
    inp, gt = shard_views(inp, rank, world), shard_views(gt, rank, world)
    # the CPU random draws of the step, fixed: every rank takes its slice of the eikonal points, all share the min-sdf steps
    rs = np.random.RandomState(7)
    eik = torch.from_numpy(rs.uniform(-1, 1, size=(B * P // 2, 3)).astype(np.float32))
    steps = torch.from_numpy(rs.uniform(0, 1, size=100).astype(np.float32))
    per = eik.shape[0] // world
    m._draw = lambda shape, lo, hi, dev: eik[rank * per:(rank + 1) * per].to(dev)
    m.ray_tracer._draw = lambda shape, lo, hi, dev: steps.to(dev)
    opt.zero_grad()
    out = m(inp, TP)
    lo = IDRLoss()(out, gt, TP, B // world)
    opt.backward(lo['loss'])                                                      # loss.backward() with the direct gradient sink
    opt.all_reduce_mean()                                                         # SUM over ranks ...
    opt.step()                                                                    # ... / world inside the Adam launch (lr = 0: parameters stay)
    torch.cuda.synchronize()
    return opt.flat_g.detach().cpu().clone(), {k: float(v.detach()) for k, v in lo.items()}


@pytest.mark.parametrize('cfg,world', [('small', 2), ('c4', 2), ('c4x8', 4)])
def test_ranks_reproduce_the_single_process_gradient(cfg, world):
    """('c4x8', 4): BASELINE configs[3]'s 16384-ray batch sharded over four ranks -- every rank takes two 2048-px views, four processes on the one
    GPU (gloo transport): the rank-averaged gradient equals the single-process gradient of the whole 16384-ray step."""
    ref, ref_losses = run_step(0, 1, cfg)                                            # whole batch, no process group
    with tempfile.TemporaryDirectory() as td:
        script = os.path.join(td, 'worker.py')
        open(script, 'w').write(WORKER.format(root=ROOT))
        port = str(29500 + os.getpid() % 2000)
        outs = [os.path.join(td, 'r%d.pt' % r) for r in range(world)]
        env = dict(os.environ, OMP_NUM_THREADS='2')
        procs = [subprocess.Popen([sys.executable, script, str(r), str(world), outs[r], port, cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
                 for r in range(world)]
        logs = [p.communicate(timeout=900)[0].decode(errors='replace') for p in procs]
        assert all(p.returncode == 0 for p in procs), '\n'.join(logs)[-3000:]
        res = [torch.load(o) for o in outs]
    for r in range(1, world):
        assert torch.equal(res[0]['flat'], res[r]['flat'])                          # every rank holds the same averaged gradient
    g, scale = res[0]['flat'], float(ref.abs().max())
    dev = float((g - ref).abs().max()) / scale
    print('%s, %d ranks: max |rank-averaged gradient - single-process gradient| = %.3g of the largest entry' % (cfg, world, dev))
    assert dev <= 2e-5 + 1e-9 / scale, dev
    # the rank losses average to the single-process loss (exactly so for the count-normalised terms thanks to the global counts)
    for k in ('loss', 'rgb_loss', 'eikonal_loss', 'depth_loss', 'feat_loss', 'surf_loss'):
        avg = sum(r_['losses'][k] for r_ in res) / world
        assert abs(avg - ref_losses[k]) <= 2e-5 * max(1.0, abs(ref_losses[k])), (k, avg, ref_losses[k])
