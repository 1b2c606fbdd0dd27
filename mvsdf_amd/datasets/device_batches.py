"""Training batches assembled on the device: what SceneDataset.__getitem__ + collate_fn give (reference code/datasets/scene_dataset.py:107-203,
idr_train.py:253-262), built by ONE HIP launch per step (csrc/batch_kernels.hip::mvsdf_batch_gather) from pools that stay on the device.

The reference's loop waits for the GPU several times per step before any model work: every item makes pageable host-to-device copies (the depth
selection and the source-view ids), the host-resident rgb / uv / masks are copied by the loop's .cuda() calls, and each epoch draws a CPU randperm over
all pixels.  Here the pools are built ONCE from the dataset's own host tensors (so the values are bit-identical by construction), the epoch's pixel
sample is a device randperm, the epoch's view order a host randperm copied once from pinned memory, and nothing on the per-step path synchronises
the host with the GPU.  Every step gets fresh output tensors from torch's caching allocator: a batch a queued step still reads is never overwritten.

Yields (indices, model_input, ground_truth) like the reference's DataLoader: indices a host LongTensor, everything else on the device with the keys,
shapes, dtypes and memory layouts of collate_fn (feat [B,32,h,w] channels-last, feat_src [B,V,32,h,w] with channel stride 1).  The dicts share
their depths / depth_cams / size / center / cam / src_cams tensors (collate_fn stacks the same values twice)."""
import ctypes as C

import torch

from .. import _lib
from .._lib import check, lib


BatchArgs = _lib.STRUCTS['MvsdfBatchArgs']


def source_table(dataset):
    """[n, num_src] int64: the source views of every view from pair.txt, as SceneDataset.__getitem__ picks them (scene_dataset.py:135-136)."""
    pair = dataset.pair
    rows = []
    for i in range(len(dataset)):
        src_ids = pair[pair['id_list'][i]]['pair']
        row = [pair[s]['index'] for s in src_ids][:dataset.num_src]
        if len(row) != dataset.num_src:
            raise ValueError('view %d has %d source views in pair.txt, %d needed' % (i, len(row), dataset.num_src))
        rows.append(row)
    return torch.tensor(rows, dtype=torch.int64).reshape(len(dataset), dataset.num_src)


class DeviceBatches:
    """Batches of `batch_size` views x `num_pixels` pixels (-1: whole images, change_sampling_idx(-1)) of a SceneDataset, drop_last like the reference's
    DataLoader.  `seed` seeds this object's own two generators (host: the view order; device: the pixel sample); the model's draws are not touched."""

    def __init__(self, dataset, batch_size, num_pixels=-1, seed=0):
        if getattr(dataset, 'sel_depth_num', 1) != 1:
            raise NotImplementedError('DeviceBatches: sel_depth_num != 1 (the reference uses 1: the view\'s own depth map)')
        if getattr(dataset, 'train_cameras', False):
            raise NotImplementedError('DeviceBatches: train_cameras')
        n = len(dataset)
        if not 1 <= batch_size <= n:
            raise ValueError('batch_size %d for %d views' % (batch_size, n))
        feats = dataset.feats
        dev = feats.device
        if dev.type != 'cuda' or not feats.is_contiguous(memory_format=torch.channels_last) or feats.shape[1] % 4:
            raise ValueError('DeviceBatches: the dataset\'s features must be a channels-last device tensor')
        self.dataset, self.batch_size, self.num_pixels, self.device = dataset, batch_size, num_pixels, dev
        self.n, self.num_src = n, dataset.num_src
        self.img_res, self.total_pixels = dataset.img_res, dataset.total_pixels
        self.n_batches = n // batch_size
        # the pools, from the dataset's own tensors (one copy each, here)
        self.rgb = torch.stack(dataset.rgb_images).to(dev).contiguous()
        self.omask = torch.stack(dataset.object_masks).to(dev).contiguous()
        self.pmask = torch.stack(dataset.perfect_masks).to(dev).contiguous() if hasattr(dataset, 'perfect_masks') else None
        self.pose = torch.stack(dataset.pose_all).to(dev).contiguous()
        self.intrinsics = torch.stack(dataset.intrinsics_all).to(dev).contiguous()
        self.cams_hd = dataset.cams_hd.to(dev).contiguous()
        self.depth_cams = dataset.depth_cams.to(dev).contiguous()
        self.depths = dataset.depths.to(dev).contiguous()
        self.size = dataset.size.to(dev).reshape(1).contiguous()
        self.center = dataset.center.to(dev).contiguous()
        self.src = source_table(dataset).to(dev)
        self.feats = feats
        assert self.rgb.shape == (n, self.total_pixels, 3) and self.omask.dtype == torch.bool
        self.gen_host = torch.Generator().manual_seed(seed)
        self.gen_dev = torch.Generator(device=dev).manual_seed(seed)
        self.sampling_idx = None                 # the epoch's pixel ids (device int64 [num_pixels]) or None (whole images)
        self.epoch_views = None                  # the epoch's view order (host int64 [n_batches * batch_size])
        self._views_dev = None
        if lib().mvsdf_batch_args_bytes() != C.sizeof(BatchArgs):
            raise _lib.MvsdfError('MvsdfBatchArgs: %d bytes in the library, %d in the binding' % (lib().mvsdf_batch_args_bytes(), C.sizeof(BatchArgs)))

    def __len__(self):
        return self.n_batches

    def new_epoch(self):
        """Draw the epoch's pixel sample (device randperm) and view order (host randperm, drop_last; copied once from pinned memory, no wait)."""
        if self.num_pixels == -1:
            self.sampling_idx = None
        else:
            self.sampling_idx = torch.randperm(self.total_pixels, device=self.device, generator=self.gen_dev)[:self.num_pixels]
        perm = torch.randperm(self.n, generator=self.gen_host)[:self.n_batches * self.batch_size]
        self.epoch_views = perm
        self._views_dev = perm.pin_memory().to(self.device, non_blocking=True)

    def __iter__(self):
        """One epoch: new draws, then one gather per step on the current stream, in line with the steps.  (A side stream one step ahead was measured
        slower at c2, 2.06 against 1.87 ms per step: the gather's workgroups take the CUs k_sphere_trace runs on; DESIGN.md, training command.)"""
        self.new_epoch()
        B = self.batch_size
        for i in range(self.n_batches):
            yield self.batch(self.epoch_views[i * B:(i + 1) * B], self._views_dev[i * B:(i + 1) * B], self.sampling_idx)

    def batch(self, indices, views_dev=None, sampling_idx=None):
        """One batch of the views `indices` (host LongTensor; views_dev: the same ids on the device, copied here -- a wait -- when not given) at the pixel
        ids `sampling_idx` (device int64, or None: whole images) -> (indices, model_input, ground_truth)."""
        indices = torch.as_tensor(indices, dtype=torch.int64)
        if indices.numel() < 1 or int(indices.min()) < 0 or int(indices.max()) >= self.n:
            raise ValueError('DeviceBatches.batch: view ids must lie in [0, %d)' % self.n)
        if views_dev is None:
            views_dev = indices.to(self.device)
        B, V, dev = int(indices.numel()), self.num_src, self.device
        P = self.total_pixels if sampling_idx is None else int(sampling_idx.numel())
        if sampling_idx is not None and (sampling_idx.device != dev or sampling_idx.dtype != torch.int64 or not sampling_idx.is_contiguous()):
            raise ValueError('sampling_idx: a contiguous int64 tensor on %s expected' % dev)
        nc, fh, fw = self.feats.shape[1:]
        f32 = dict(dtype=torch.float32, device=dev)
        rgb = torch.empty(B, P, 3, **f32)
        uv = torch.empty(B, P, 2, **f32)
        omask = torch.empty(B, P, dtype=torch.bool, device=dev)
        pmask = torch.empty(B, P, dtype=torch.bool, device=dev) if self.pmask is not None else None
        pose, intr = torch.empty(B, 4, 4, **f32), torch.empty(B, 4, 4, **f32)
        cam, src_cams = torch.empty(B, 2, 4, 4, **f32), torch.empty(B, V, 2, 4, 4, **f32)
        depths = torch.empty((B, 1) + tuple(self.depths.shape[1:]), **f32)
        depth_cams = torch.empty(B, 1, 2, 4, 4, **f32)
        size, center = torch.empty(B, **f32), torch.empty(B, 3, **f32)
        feat = torch.empty(B, fh, fw, nc, **f32).permute(0, 3, 1, 2)                       # channels-last [B,32,h,w]
        feat_src = torch.empty(B, V, fh, fw, nc, **f32).permute(0, 1, 4, 2, 3)            # [B,V,32,h,w], channel stride 1
        p = lambda t: t.data_ptr() if t is not None else None
        a = BatchArgs(B=B, n=self.n, num_src=V, P=P, img_w=self.img_res[1], total_pixels=self.total_pixels,
                      depth_floats=self.depths[0].numel(), fmap_floats=self.feats[0].numel(),
                      views=p(views_dev), pix=p(sampling_idx), src=p(self.src), rgb=p(self.rgb), omask=p(self.omask), pmask=p(self.pmask),
                      pose=p(self.pose), intrinsics=p(self.intrinsics), cams_hd=p(self.cams_hd), depth_cams=p(self.depth_cams), depths=p(self.depths),
                      size=p(self.size), center=p(self.center), feats=p(self.feats), o_rgb=p(rgb), o_uv=p(uv), o_omask=p(omask), o_pmask=p(pmask),
                      o_pose=p(pose), o_intrinsics=p(intr), o_cam=p(cam), o_src_cams=p(src_cams), o_depths=p(depths), o_depth_cams=p(depth_cams),
                      o_size=p(size), o_center=p(center), o_feat=p(feat), o_feat_src=p(feat_src))
        stream = torch.cuda.current_stream(dev)
        check(lib().mvsdf_batch_gather(C.byref(a), C.c_void_p(stream.cuda_stream)), 'mvsdf_batch_gather')
        model_input = {'object_mask': omask, 'uv': uv, 'intrinsics': intr}
        if pmask is not None:
            model_input['perfect_mask'] = pmask
        model_input['pose'] = pose
        ground_truth = {'rgb': rgb, 'depths': depths, 'depth_cams': depth_cams, 'size': size, 'center': center, 'feat': feat, 'feat_src': feat_src,
                        'cam': cam, 'src_cams': src_cams}
        for k in ('depths', 'depth_cams', 'size', 'center', 'cam', 'src_cams'):
            model_input[k] = ground_truth[k]
        return indices, model_input, ground_truth
