"""SceneDataset with the reference's interface (code/datasets/scene_dataset.py:16-242), needing only numpy, PIL and torch.

A scene directory holds image_hd/ and mask_hd/ (images, sorted by name), depth/<i:03>.pfm (MVS depth maps), cameras_hd.npz (world_mat_i,
scale_mat_i) and optionally pmask/ (perfect masks); beside it, ../pair.txt and ../cam_<8-digit id>_flow3.txt (MVSNet cameras at depth-map
resolution).  The constructor loads them, resizes the images to rgb_2xd (feat_img_scale times the depth-map size, bilinear, as the reference)
with ImageNet normalisation, and runs FeatExt once per scene on the device (features.extract_features).  The features stay on the device,
channels-last, and items slice them: feat [32,h,w] and feat_src [num_src,32,h,w] are device tensors whose channel stride is 1, the layout
k_feat_corr reads best.  Depth maps and cameras are device-resident too.

feat_weights_only=False loads a trusted checkpoint that holds pickled objects besides tensors (see FeatExt.from_checkpoint).

Differences from the reference: train_cameras=True and the IDR_ONLY_CAM branch raise NotImplementedError (the reference disables camera
training, exp_runner.py:40); collate_fn stacks feat / feat_src into the same shapes in that channels-last layout.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from .. import features
from ..model import conf
from ..utils import io as sio


class SceneDataset(torch.utils.data.Dataset):
    """Dataset for a class of objects, where each datapoint is a SceneInstanceDataset."""

    def __init__(self, data_dir, train_cameras=False, cam_file=None, feat_ckpt='utils/vismvsnet.pt', device='cuda', feat_weights_only=True):
        if train_cameras:
            raise NotImplementedError('train_cameras=True: camera training is disabled in the reference (exp_runner.py:40) and not built')
        if os.environ.get('IDR_USE_ENV', '0') == '1' and os.environ.get('IDR_ONLY_CAM', '0') == '1':
            raise NotImplementedError('the IDR_ONLY_CAM branch of the reference dataset is not built')
        self.instance_dir = data_dir
        self.only_cam = False
        assert os.path.exists(self.instance_dir), "Data directory is empty"
        self.sampling_idx = None
        self.train_cameras = train_cameras
        dev = torch.device(device)

        image_paths = sorted(sio.glob_imgs('{0}/image_hd'.format(self.instance_dir)))
        mask_paths = sorted(sio.glob_imgs('{0}/mask_hd'.format(self.instance_dir)))
        self.n_images = len(image_paths)

        self.cam_file = '{0}/cameras_hd.npz'.format(self.instance_dir)
        if cam_file is not None:
            self.cam_file = '{0}/{1}'.format(self.instance_dir, cam_file)
        camera_dict = np.load(self.cam_file)
        scale_mats = [camera_dict['scale_mat_%d' % idx].astype(np.float32) for idx in range(self.n_images)]
        world_mats = [camera_dict['world_mat_%d' % idx].astype(np.float32) for idx in range(self.n_images)]
        self.intrinsics_all, self.pose_all = [], []
        for scale_mat, world_mat in zip(scale_mats, world_mats):
            P = (world_mat @ scale_mat)[:3, :4]
            intrinsics, pose = sio.load_K_Rt_from_P(None, P)
            self.intrinsics_all.append(torch.from_numpy(intrinsics).float())
            self.pose_all.append(torch.from_numpy(pose).float())

        self.rgb_images = []
        for path in image_paths:
            rgb = sio.load_rgb(path)
            input_res = rgb.shape[-2:]
            self.rgb_images.append(torch.from_numpy(rgb.reshape(3, -1).transpose(1, 0)).float())
        self.img_res = input_res
        self.total_pixels = self.img_res[0] * self.img_res[1]
        self.object_masks = [torch.from_numpy(sio.load_mask(p).reshape(-1)).bool() for p in mask_paths]

        self.pair = sio.load_pair(f'{self.instance_dir}/../pair.txt')
        self.num_src = 2  # as the reference
        self.depths = torch.stack([torch.from_numpy(np.ascontiguousarray(sio.load_pfm(f'{self.instance_dir}/depth/{i:03}.pfm'))).to(torch.float32)
                                   for i in range(self.n_images)], dim=0).unsqueeze(1)
        self.depth_cams = torch.stack([torch.from_numpy(sio.load_cam(f'{self.instance_dir}/../cam_{self.pair["id_list"][i].zfill(8)}_flow3.txt',
                                                                     256, 1)).to(torch.float32) for i in range(self.n_images)], dim=0)
        self.feat_img_scale = conf.feat_img_scale
        self.cams_hd = torch.stack([sio.scale_camera(self.depth_cams[i], self.feat_img_scale) for i in range(self.n_images)])
        fh, fw = self.depths.size()[-2] * self.feat_img_scale, self.depths.size()[-1] * self.feat_img_scale
        self.rgb_2xd = torch.stack([
            F.interpolate(self.rgb_images[i].permute(1, 0).view(1, 3, *self.img_res), size=(fh, fw), mode='bilinear', align_corners=False)[0]
            if (self.img_res[0], self.img_res[1]) != (fh, fw) else self.rgb_images[i].permute(1, 0).view(3, *self.img_res)
            for i in range(self.n_images)], dim=0)  # v3hw
        mean = torch.tensor([0.485, 0.456, 0.406]).float()
        std = torch.tensor([0.229, 0.224, 0.225]).float()
        self.rgb_2xd = (self.rgb_2xd / 2 + 0.5 - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)

        self.size = torch.from_numpy(scale_mats[0]).float()[0, 0] * 2
        self.center = torch.from_numpy(scale_mats[0]).float()[:3, 3]
        self.sel_depth_num = 1  # as the reference

        uv = np.mgrid[0:self.img_res[0], 0:self.img_res[1]].astype(np.int32)
        uv = torch.from_numpy(np.flip(uv, axis=0).copy()).float()
        self.uv = uv.reshape(2, -1).transpose(1, 0)

        # device-resident per-scene constants
        self.depths, self.depth_cams, self.cams_hd = self.depths.to(dev), self.depth_cams.to(dev), self.cams_hd.to(dev)
        self.size, self.center = self.size.to(dev), self.center.to(dev)
        self.feat_ext = features.FeatExt.from_checkpoint(feat_ckpt, weights_only=feat_weights_only).to(dev).eval()
        for p in self.feat_ext.parameters():
            p.requires_grad = False
        self.feats = features.extract_features(self.feat_ext, self.rgb_2xd, batch=20)      # [n,32,h,w] channels-last on the device
        self.feat_ext.release_workspace()                 # the activations of a batch of 20 views (GBs at DTU size) are not needed again

        if os.path.exists(f'{self.instance_dir}/pmask'):
            pmask_dir = f'{self.instance_dir}/pmask'
            print('find perfect mask dir:', pmask_dir)
            self.perfect_masks = [torch.from_numpy(sio.load_mask(p).reshape(-1)).bool() for p in sorted(sio.glob_imgs(pmask_dir))]

    def __len__(self):
        return self.n_images

    def __getitem__(self, idx):
        sample = {
            "object_mask": self.object_masks[idx],
            "uv": self.uv,
            "intrinsics": self.intrinsics_all[idx],
        }
        if hasattr(self, 'perfect_masks'):
            sample['perfect_mask'] = self.perfect_masks[idx]
        ground_truth = {"rgb": self.rgb_images[idx]}
        if self.sampling_idx is not None:
            ground_truth["rgb"] = self.rgb_images[idx][self.sampling_idx, :]
            sample["object_mask"] = self.object_masks[idx][self.sampling_idx]
            sample["uv"] = self.uv[self.sampling_idx, :]
            if hasattr(self, 'perfect_masks'):
                sample["perfect_mask"] = self.perfect_masks[idx][self.sampling_idx]
        if not self.train_cameras:
            sample["pose"] = self.pose_all[idx]

        views = [i for i in range(self.n_images) if i != idx]
        sel_depth_idxs = np.sort(np.concatenate([np.random.choice(views, self.sel_depth_num - 1, replace=False), [idx]]))
        dsel = torch.from_numpy(sel_depth_idxs.astype(np.int64)).to(self.depths.device)
        ground_truth['depths'] = self.depths[dsel]
        ground_truth['depth_cams'] = self.depth_cams[dsel]
        ground_truth['size'] = self.size
        ground_truth['center'] = self.center

        src_ids = self.pair[self.pair['id_list'][idx]]['pair']
        src_idxs = [self.pair[src_id]['index'] for src_id in src_ids][:self.num_src]
        sel = torch.tensor(src_idxs, dtype=torch.int64, device=self.feats.device)
        ground_truth["feat"] = self.feats[idx]                                                        # a view: no copy
        ground_truth["feat_src"] = self.feats[sel].contiguous(memory_format=torch.channels_last)     # a device gather
        ground_truth["cam"] = self.cams_hd[idx]
        ground_truth["src_cams"] = self.cams_hd[sel]
        for attr in ['depths', 'depth_cams', 'size', 'center', 'cam', 'src_cams']:
            sample[attr] = ground_truth[attr]
        return idx, sample, ground_truth

    def collate_fn(self, batch_list):
        """Stack the items' dicts (scene_dataset.py:189-203); feat [B,32,h,w] and feat_src [B,V,32,h,w] come out with channel stride 1."""
        all_parsed = []
        for entry in zip(*batch_list):
            if type(entry[0]) is dict:
                ret = {}
                for k in entry[0].keys():
                    ret[k] = torch.stack([obj[k] for obj in entry])
                if 'feat' in ret:
                    ret['feat'] = ret['feat'].contiguous(memory_format=torch.channels_last)
                if 'feat_src' in ret:
                    ret['feat_src'] = ret['feat_src'].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
                all_parsed.append(ret)
            else:
                all_parsed.append(torch.LongTensor(entry))
        return tuple(all_parsed)

    def change_sampling_idx(self, sampling_size):
        if sampling_size == -1:
            self.sampling_idx = None
        else:
            self.sampling_idx = torch.randperm(self.total_pixels)[:sampling_size]

    def get_scale_mat(self):
        return np.load(self.cam_file)['scale_mat_0']

    def get_gt_pose(self, scaled=False):
        camera_dict = np.load(self.cam_file)
        world_mats = [camera_dict['world_mat_%d' % idx].astype(np.float32) for idx in range(self.n_images)]
        scale_mats = [camera_dict['scale_mat_%d' % idx].astype(np.float32) for idx in range(self.n_images)]
        pose_all = []
        for scale_mat, world_mat in zip(scale_mats, world_mats):
            P = (world_mat @ scale_mat if scaled else world_mat)[:3, :4]
            pose_all.append(torch.from_numpy(sio.load_K_Rt_from_P(None, P)[1]).float())
        return torch.stack(pose_all, 0)
