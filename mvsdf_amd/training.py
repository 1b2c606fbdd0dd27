"""The training command (reference code/training/exp_runner.py + idr_train.py::IDRTrainRunner) on this project's pieces.

Same flags, configuration, schedule, checkpoint tree and log lines as the reference, with three differences in how a step is fed and reported:
  * batches come from datasets.device_batches.DeviceBatches (one HIP launch per step, no host wait) instead of SceneDataset + DataLoader + .cuda();
  * the optimiser is optim.FlatAdam (grad-norm + clip + Adam in one launch), stepped with zero_grad=True like bench.py;
  * the reference's three log lines per step are printed LAGGED: the six loss scalars and the gradient norm go into a pinned slot with an event, and a
    line is printed once its event has completed (queried, never waited for).  The lines are flushed at checkpoint time and at the end of the run.
So the step loop  zero_grad -> batch -> model -> IDRLoss -> backward -> step  never waits on the GPU (with the deferred step, IDRNetwork's default).

Directory tree (idr_train.py:37-75): <exps_root>/<exps_folder>/<train.expname>_<expname>/<timestamp>/{plots, checkpoints/{Model,Optimizer,Scheduler}Parameters}.
plots/ holds surface_<epoch>.obj at every plot epoch and, every fourth, rendering_<epoch>.png (output above ground truth) and depth_<epoch>.png; the
reference's plotly HTML is left out.  Camera training (train_cameras) is switched off in the reference (exp_runner.py:40) and not built."""
import argparse
import collections
import os
import random
import sys
import warnings
from datetime import datetime

import numpy as np
import torch

from . import checkpoint as ckpt
from .utils import config as cfg

LOSS_KEYS = ('loss', 'rgb_loss', 'eikonal_loss', 'feat_loss', 'depth_loss', 'surf_loss')


# ---- configuration
def fraction(s):
    """'a/b' -> a / b as the reference parses it (idr_train.py:116-117, 153-155)."""
    a, b = str(s).split('/')
    return int(a) / int(b)


def sched_milestones(conf, nepochs):
    """MultiStepLR milestones: int(nepochs * a / b) for every 'a/b' of train.sched_milestones (idr_train.py:114-118)."""
    train = conf.get_config('train')
    return [int(nepochs * float(fraction(v))) for v in train.get('sched_milestones', [])]


def sched_factor(conf):
    return float(conf.get_config('train').get('sched_factor', 0.0))


def plot_freq(conf, nepochs):
    """int(a / b * nepochs) of train.plot_freq (idr_train.py:153-156)."""
    return int(fraction(conf.get_string('train.plot_freq')) * nepochs)


def schedule_module():
    """The schedule module (model/conf.py or its IDR_USE_ENV / IDR_CONF override) exactly as IDRLoss and the model read it."""
    from .model import loss
    return loss.conf


# ---- the exps tree
def latest_timestamp(expdir):
    """The newest timestamp directory of an experiment (sorted name order, idr_train.py:33-38), or None."""
    if not os.path.exists(expdir):
        return None
    ts = os.listdir(expdir)
    return sorted(ts)[-1] if ts else None


def resolve_continue(expdir, is_continue, timestamp):
    """-> (is_continue, timestamp) as idr_train.py:31-45 decides them: --is_continue with 'latest' picks the newest run, and continues nothing without one."""
    if is_continue and timestamp == 'latest':
        ts = latest_timestamp(expdir)
        return (ts is not None), ts
    return is_continue, timestamp


# ---- logging
def step_lines(expname, epoch, nepochs, data_index, n_batches, values, grad_norm, grad_cap, lr):
    """The reference's three lines of one step (idr_train.py:289-313) from host numbers: values = the six loss scalars in LOSS_KEYS order."""
    lines = ['grad norm: %s' % (float(grad_norm),)]
    if grad_cap is not None:
        lines.append('grad cap: %s' % (grad_cap,))
    v = dict(zip(LOSS_KEYS, (float(x) for x in values)))
    lines.append(' '.join([f"{expname} [{epoch}/{nepochs}] ({data_index}/{n_batches}):",
                           f"loss = {v['loss']:.4f},", f"rgb_loss = {v['rgb_loss']:.4f},", f"eikonal_loss = {v['eikonal_loss']:.4f},",
                           f"feat_loss = {v['feat_loss']:.4f},", f"depth_loss = {v['depth_loss']:.4f},", f"surf_loss = {v['surf_loss']:.4f},",
                           f"lr = {lr}"]))
    return lines


class LaggedLog:
    """Per-step scalars copied into pinned slots behind the step, printed once their copy has landed.  push() enqueues one device-side gather + one
    asynchronous copy + an event; poll() prints the lines whose events have completed (query only); flush() waits for the rest.  A slot is reused only
    after it was printed; when every slot is still in flight a new one is added.  `records` keeps (epoch, data_index, values, grad_norm) per step."""

    def __init__(self, printer=print):
        self.printer = printer
        self.pending = collections.deque()
        self.free = []
        self.records = []

    def push(self, loss_out, grad_norm, meta):
        vals = torch.cat([loss_out[k].detach().reshape(-1)[:1].float() for k in LOSS_KEYS] + [grad_norm.detach().reshape(1).float()])
        buf = self.free.pop() if self.free else torch.empty(len(LOSS_KEYS) + 1, dtype=torch.float32).pin_memory()
        buf.copy_(vals, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev, buf, meta))

    def _emit(self, buf, meta):
        v = buf.tolist()
        expname, epoch, nepochs, data_index, n_batches, grad_cap, lr = meta
        self.records.append((epoch, data_index, v[:len(LOSS_KEYS)], v[len(LOSS_KEYS)]))
        for line in step_lines(expname, epoch, nepochs, data_index, n_batches, v[:len(LOSS_KEYS)], v[len(LOSS_KEYS)], grad_cap, lr):
            self.printer(line)
        self.free.append(buf)

    def poll(self):
        while self.pending and self.pending[0][0].query():
            _, buf, meta = self.pending.popleft()
            self._emit(buf, meta)

    def flush(self):
        while self.pending:
            ev, buf, meta = self.pending.popleft()
            ev.synchronize()
            self._emit(buf, meta)


# ---- images (torchvision is not used)
def make_grid(imgs, nrow=8, padding=2, normalize=False, scale_each=False, pad_value=0.0):
    """torchvision.utils.make_grid on a numpy [N, C, H, W] batch -> [C, H', W'] (one image: returned as it is, after the optional normalisation)."""
    imgs = np.array(imgs, dtype=np.float32)
    if imgs.shape[1] == 1:
        imgs = np.repeat(imgs, 3, axis=1)
    if normalize:
        def norm(t):
            lo, hi = float(t.min()), float(t.max())
            np.clip(t, lo, hi, out=t)
            t -= lo
            t /= max(hi - lo, 1e-5)
        if scale_each:
            for t in imgs:
                norm(t)
        else:
            norm(imgs)
    n, c, h, w = imgs.shape
    if n == 1:
        return imgs[0]
    xmaps = min(nrow, n)
    ymaps = int(np.ceil(n / xmaps))
    hh, ww = h + padding, w + padding
    grid = np.full((c, hh * ymaps + padding, ww * xmaps + padding), pad_value, dtype=np.float32)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid[:, y * hh + padding:y * hh + padding + h, x * ww + padding:x * ww + padding + w] = imgs[k]
            k += 1
    return grid


def save_png(grid, path):
    from PIL import Image
    Image.fromarray((grid.transpose(1, 2, 0) * 255).astype(np.uint8)).save(path)


def camera_depth(points, pose):
    """rend_util.get_depth (rend_util.py:164-181), 4 x 4 pose branch: the z of each point in the camera frame.  points [B, N, 3], pose [B, 4, 4] -> [B, N, 1]."""
    b, n, _ = points.shape
    hom = torch.cat((points, torch.ones((b, n, 1), dtype=points.dtype, device=points.device)), dim=2).permute(0, 2, 1)
    return torch.inverse(pose).bmm(hom)[:, 2, :][:, :, None]


@torch.no_grad()
def render_full(model, model_input, total_pixels, n_pixels=10000):
    """The reference's plot render (idr_train.py:221-234): every chunk through IDRNetwork in eval mode -> merged points / rgb_values / network_object_mask."""
    from .utils import general as gu
    res = []
    for s in gu.split_input(model_input, total_pixels, n_pixels=n_pixels):
        out = model(s)
        res.append({'points': out['points'].detach(), 'rgb_values': out['rgb_values'].detach(),
                    'network_object_mask': out['network_object_mask'].detach()})
    return gu.merge_output(res, total_pixels, model_input['uv'].shape[0])


def plot_images(outputs, model_input, rgb_gt, path, epoch, img_res, plot_nimgs, max_depth):
    """plots.py:12-32, 342-373: rendering_<epoch>.png (output above ground truth) and depth_<epoch>.png (max_depth where nothing was hit)."""
    from .utils.plots import lin2img
    b, n = rgb_gt.shape[0], rgb_gt.shape[1]
    hit = outputs['network_object_mask']
    points = outputs['points'].reshape(b, n, 3)
    depth = torch.ones(b * n, dtype=torch.float32, device=points.device) * max_depth
    depth[hit] = camera_depth(points, model_input['pose']).reshape(-1)[hit]
    depth = depth.reshape(b, n, 1)
    rgb = (outputs['rgb_values'].reshape(b, n, 3) + 1.0) / 2.0
    gt = (rgb_gt + 1.0) / 2.0
    both = lin2img(torch.cat((rgb, gt), dim=0), img_res).cpu().numpy()
    save_png(make_grid(both, nrow=plot_nimgs), os.path.join(path, 'rendering_%d.png' % epoch))
    save_png(make_grid(lin2img(depth, img_res).cpu().numpy(), nrow=plot_nimgs, normalize=True, scale_each=True), os.path.join(path, 'depth_%d.png' % epoch))


# ---- the runner
class IDRTrainRunner:
    """idr_train.py::IDRTrainRunner.  kwargs: conf, data_dir, batch_size, nepochs, expname, gpu_index, exps_folder_name, is_continue, timestamp,
    checkpoint, train_cameras (False only) and, beyond the reference, exps_root (default '../'), seed (None: unseeded), feat_ckpt (None: the
    dataset's default), printer (the log's print function)."""

    def __init__(self, **kwargs):
        from .datasets.device_batches import DeviceBatches
        from .datasets.scene_dataset import SceneDataset
        from .model.implicit_differentiable_renderer import IDRNetwork
        from .model.loss import IDRLoss
        from .optim import FlatAdam
        if kwargs.get('train_cameras', False):
            raise NotImplementedError('train_cameras: camera training is disabled in the reference (exp_runner.py:40) and not built')
        torch.set_default_dtype(torch.float32)
        self.conf = cfg.load_conf(kwargs['conf'])
        self.data_dir = kwargs['data_dir']
        self.batch_size = kwargs['batch_size']
        self.nepochs = kwargs['nepochs']
        self.exps_folder_name = kwargs.get('exps_folder_name', 'exps')
        self.exps_root = kwargs.get('exps_root', '../')
        self.train_cameras = False
        self.printer = kwargs.get('printer', print)
        seed = kwargs.get('seed')
        if seed is not None:
            torch.manual_seed(seed)                               # the CPU generator and every device's
            np.random.seed(seed)
            random.seed(seed)
        self.plot_freq = plot_freq(self.conf, self.nepochs)
        if self.plot_freq < 1:
            raise ValueError('train.plot_freq x nepochs = %d: at least one epoch between plots is needed' % self.plot_freq)
        self.expname = self.conf.get_string('train.expname') + '_' + kwargs['expname']
        self.expdir = os.path.join(self.exps_root, self.exps_folder_name, self.expname)
        is_continue, timestamp = resolve_continue(self.expdir, kwargs.get('is_continue', False), kwargs.get('timestamp', 'latest'))

        os.makedirs(self.expdir, exist_ok=True)
        self.timestamp = '{:%Y_%m_%d_%H_%M_%S}'.format(datetime.now())
        self.plots_dir = os.path.join(self.expdir, self.timestamp, 'plots')
        self.checkpoints_path = os.path.join(self.expdir, self.timestamp, 'checkpoints')
        for sub in (ckpt.MODEL_SUBDIR, ckpt.OPTIMIZER_SUBDIR, ckpt.SCHEDULER_SUBDIR):
            os.makedirs(os.path.join(self.checkpoints_path, sub), exist_ok=True)
        os.makedirs(self.plots_dir, exist_ok=True)

        self.printer('shell command : {0}'.format(' '.join(sys.argv)))
        self.printer('Loading data ...')
        dataset_conf = dict(self.conf.get_config('dataset')) if 'dataset' in self.conf else {}
        if kwargs.get('feat_ckpt') is not None:
            dataset_conf['feat_ckpt'] = kwargs['feat_ckpt']
        self.train_dataset = SceneDataset(self.data_dir, False, **dataset_conf)
        self.printer('Finish loading data ...')
        self.num_pixels = self.conf.get_int('train.num_pixels')
        batch_seed = seed if seed is not None else random.SystemRandom().randrange(1 << 62)
        self.batches = DeviceBatches(self.train_dataset, self.batch_size, self.num_pixels, seed=batch_seed)
        self.plot_rng = np.random.RandomState(batch_seed % (1 << 32))   # the plot view (the reference's shuffled plot DataLoader)

        self.model = IDRNetwork(conf=self.conf.get_config('model')).cuda()
        loss_conf = dict(self.conf.get_config('loss')) if 'loss' in self.conf else {}
        self.loss = IDRLoss(**loss_conf)
        self.lr = self.conf.get_float('train.learning_rate') * self.batch_size
        self.printer('batch size scaled lr: %s' % (self.lr,))
        self.optimizer = FlatAdam(self.model.parameters(), lr=self.lr)
        self.sched_milestones = sched_milestones(self.conf, self.nepochs)
        self.sched_factor = sched_factor(self.conf)
        self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, self.sched_milestones, gamma=self.sched_factor)

        self.start_epoch = 0
        if is_continue:
            old = os.path.join(self.expdir, timestamp, 'checkpoints')
            self.start_epoch = ckpt.load_checkpoints(old, self.model, self.optimizer, self.scheduler, checkpoint=kwargs.get('checkpoint', 'latest'))

        self.total_pixels = self.train_dataset.total_pixels
        self.img_res = self.train_dataset.img_res
        self.n_batches = len(self.batches)
        self.plot_conf = self.conf.get_config('plot')
        self.log = LaggedLog(self.printer)

    def save_checkpoints(self, epoch):
        ckpt.save_checkpoints(self.checkpoints_path, epoch, self.model, self.optimizer, self.scheduler)

    def _lr_for_log(self):
        with warnings.catch_warnings():                         # the reference's scheduler.get_lr()[0] (idr_train.py:313), its milestone quirk included
            warnings.simplefilter('ignore')
            return self.scheduler.get_lr()[0]

    def plot_epoch(self, epoch, full=False):
        from . import mesh
        self.model.eval()
        if full:
            view = int(self.plot_rng.randint(len(self.train_dataset)))
            _, model_input, ground_truth = self.batches.batch(torch.tensor([view]))
            outputs = render_full(self.model, model_input, self.total_pixels)
            plot_images(outputs, model_input, ground_truth['rgb'], self.plots_dir, epoch, self.img_res, self.plot_conf.get_int('plot_nimgs'),
                        self.plot_conf.get_float('max_depth'))
        m = mesh.surface_mesh(self.model, self.plot_conf.get_int('resolution'), colors=False)
        if m is not None:
            m.export(os.path.join(self.plots_dir, 'surface_%d.obj' % epoch))
        self.model.train()

    def train_epoch(self, epoch):
        sched = schedule_module()
        tp = epoch / self.nepochs
        cap = sched.grad_cap(tp) if (sched.phase[0] <= tp and sched.enable_grad_cap) else None
        lr = self._lr_for_log()
        for data_index, (indices, model_input, ground_truth) in enumerate(self.batches):
            self.optimizer.zero_grad()
            model_outputs = self.model(model_input, tp)
            loss_output = self.loss(model_outputs, ground_truth, tp, self.n_batches)
            self.optimizer.backward(loss_output['loss'])
            self.optimizer.step(grad_cap=cap, zero_grad=True)
            self.log.push(loss_output, self.optimizer.grad_norm(), (self.expname, epoch, self.nepochs, data_index, self.n_batches, cap, lr))
            self.log.poll()
        self.scheduler.step()

    def run(self):
        self.printer('training...')
        for epoch in range(self.start_epoch, self.nepochs + 1):
            self.train_epoch(epoch)
            if epoch % self.plot_freq == 0 and epoch != 0:
                self.log.flush()
                self.save_checkpoints(epoch)
                self.plot_epoch(epoch, full=(epoch % (self.plot_freq * 4) == 0))
        self.log.flush()


# ---- the command line (exp_runner.py)
def parser():
    p = argparse.ArgumentParser(description='Train MVSDF on one scene (the reference\'s training/exp_runner.py).')
    p.add_argument('--data_dir', type=str, default='fill_in_data_dir')
    p.add_argument('--batch_size', type=int, default=8, help='input batch size')
    p.add_argument('--nepoch', type=int, default=1800, help='number of epochs to train for')
    p.add_argument('--conf', type=str, default='./confs/mvsdf_dtu.conf')
    p.add_argument('--expname', type=str, default='test')
    p.add_argument('--gpu', type=str, default='auto', help='GPU to use: an index, or auto / ignore (the current device)')
    p.add_argument('--is_continue', default=False, action='store_true', help='If set, indicates continuing from a previous run.')
    p.add_argument('--timestamp', default='latest', type=str, help='The timestamp of the run to be used in case of continuing from a previous run.')
    p.add_argument('--checkpoint', default='latest', type=str, help='The checkpoint epoch number of the run to be used in case of continuing from a previous run.')
    p.add_argument('--exps_root', type=str, default='../', help='Directory that holds exps/ (the reference writes ../exps).')
    p.add_argument('--seed', type=int, default=None, help='Seed of every generator the step and the batches draw from (torch CPU and device, numpy).')
    p.add_argument('--feat_ckpt', type=str, default=None, help='Vis-MVSNet checkpoint for the feature extractor (SceneDataset feat_ckpt).')
    return p


def select_gpu(gpu):
    """exp_runner.py:24-29 / idr_train.py:77-78 without GPUtil: an index restricts the visible devices; 'auto' and 'ignore' keep the current device."""
    if gpu not in ('auto', 'ignore'):
        os.environ['CUDA_VISIBLE_DEVICES'] = '{0}'.format(gpu)


def main(argv=None, printer=print):
    opt = parser().parse_args(argv)
    select_gpu(opt.gpu)
    runner = IDRTrainRunner(conf=opt.conf, data_dir=opt.data_dir, batch_size=opt.batch_size, nepochs=opt.nepoch, expname=opt.expname,
                            gpu_index=opt.gpu, exps_folder_name='exps', is_continue=opt.is_continue, timestamp=opt.timestamp,
                            checkpoint=opt.checkpoint, train_cameras=False, exps_root=opt.exps_root, seed=opt.seed, feat_ckpt=opt.feat_ckpt,
                            printer=printer)
    runner.run()
    return runner
