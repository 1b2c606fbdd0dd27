"""Scene preparation: from the output of Vis-MVSNet (depth maps, three probability maps, cameras, pair.txt) to the imfunc4/ scene directory that
SceneDataset and tools/train.py read.  convert_scene follows the reference's code/datasets/vismvsnet2mvsdf.py line by line (line numbers below
are that file's) with numpy / PIL / torch in place of OpenCV and open3d:

* cameras, scale_mat, masks and depths are computed with the reference's own torch calls on the host, so they carry its bits;
* cut.ply is read by chamfer.load_points (binary) or read_ply_ascii (what a mesh editor often saves after a manual cut);
* images: cv2.resize(INTER_LINEAR) + centre crop becomes resize_bilinear_u8 + centre crop.  OpenCV rounds its interpolation weights to 1/2048, so its
  output can differ from resize_bilinear_u8's by a grey level; OpenCV is not available to this project's tests, so that is stated, not checked.
  Images are decoded by PIL (cv2.imread there; both normally sit on libjpeg) and written as RGB PNG;
* <id>_mask.png is read as PIL's 8-bit grey (cv2.IMREAD_GRAYSCALE there: the same bytes for a grey file);
* --show_range needs a viewer and is not built.

Beyond the reference: range_source='fused' runs fusion.fuse_depths, writes all_torch.ply and takes the box of the whole cloud (a scene that needs
no manual cut); range_source='clean' fuses likewise, makes the cut with cloud.clean_fused, writes all_torch.ply (the whole cloud) and cut.ply (the
cleaned cloud: a later range_source='pcd' run reproduces the box, and a person can still edit the file) and takes the box of the cleaned cloud;
fused_depth=True writes Fused.fused_depths (the cleaned ones under 'clean'), which also drops what the source views contradict, instead of the
masked depths.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from ..utils import io as sio


def pair_indices(pair):
    """pair.txt's source ids as view indices, one list per view (nearest first); sources that are not views themselves are dropped"""
    index = {vid: i for i, vid in enumerate(pair['id_list'])}
    return [[index[s] for s in pair[vid]['pair'] if s in index] for vid in pair['id_list']]


def load_mvs_output(data_root, probs=True, pair_file=None):
    """pair_file: default <data_root>/pair.txt.  -> (pair dict, cams fp64 [V,2,4,4] (load_cam(..., 256, 1, override=True), line 45), depths fp32 [V,H,W], probs fp32 [V,3,H,W] or None)"""
    pair = sio.load_pair(pair_file or os.path.join(data_root, 'pair.txt'))
    ids = [i.zfill(8) for i in pair['id_list']]
    cams = np.stack([sio.load_cam(os.path.join(data_root, 'cam_%s_flow3.txt' % i), 256, 1, override=True) for i in ids])
    depths = np.stack([np.ascontiguousarray(sio.load_pfm(os.path.join(data_root, '%s_flow3.pfm' % i))) for i in ids]).astype(np.float32)
    pr = None
    if probs:
        pr = np.stack([np.stack([np.ascontiguousarray(sio.load_pfm(os.path.join(data_root, '%s_flow%d_prob.pfm' % (i, j + 1)))) for j in range(3)])
                       for i in ids]).astype(np.float32)
    return pair, cams, depths, pr


def load_image_u8(path):
    """-> uint8 [H,W,3] RGB"""
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def resize_bilinear_u8(img, width, height, device=None):
    """uint8 [H0,W0,C] -> uint8 [height,width,C]: output pixel x reads source coordinate (x + 0.5) * W0 / width - 0.5 clamped to [0, W0-1], two taps
    per axis, value floor(v + 0.5) clamped to 0..255, computed by F.interpolate(bilinear, align_corners=False, antialias=False) in fp32 on `device`
    (default: the GPU where there is one).  Equal sizes return the input untouched."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError('resize_bilinear_u8: img must be uint8 [H, W, C]')
    if img.shape[0] == height and img.shape[1] == width:
        return img
    dev = torch.device(device) if device is not None else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    t = torch.from_numpy(np.array(img)).to(dev).permute(2, 0, 1)[None].float()
    out = F.interpolate(t, size=(int(height), int(width)), mode='bilinear', align_corners=False, antialias=False)
    out = torch.floor(out + 0.5).clamp_(0, 255).to(torch.uint8)
    return np.ascontiguousarray(out[0].permute(1, 2, 0).cpu().numpy())


def center_crop(img, width, height):
    """lines 16-23"""
    h_o, w_o = img.shape[:2]
    if w_o == width and h_o == height:
        return img
    sw, sh = (w_o - width) // 2, (h_o - height) // 2
    return img[sh:sh + height, sw:sw + width]


def read_ply_ascii(path):
    """the vertex x / y / z of an ASCII PLY -> fp64 numpy [N,3] (the vertex element must come first, as every writer puts it)"""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError('read_ply_ascii: %s is not a PLY file' % path)
    head = data[:end].decode('ascii', 'replace').splitlines()
    if not any(l.split()[:2] == ['format', 'ascii'] for l in head):
        raise ValueError('read_ply_ascii: %s is not an ASCII PLY' % path)
    elems = []
    for line in head:
        t = line.split()
        if t[:1] == ['element']:
            elems.append([t[1], int(t[2]), []])
        elif t[:1] == ['property'] and elems:
            elems[-1][2].append(t[-1] if t[1] != 'list' else None)
    if not elems or elems[0][0] != 'vertex' or not all(k in elems[0][2] for k in 'xyz'):
        raise ValueError('read_ply_ascii: %s: the first element must be vertex with x / y / z' % path)
    _, n, props = elems[0]
    body = data[data.index(b'\n', end) + 1:].split(b'\n')[:n]
    rows = np.array([l.split() for l in body], dtype=np.float64).reshape(n, len(props))
    return np.ascontiguousarray(rows[:, [props.index(k) for k in 'xyz']])


def read_points(path):
    """cut.ply in either PLY flavour -> fp64 numpy [N,3]"""
    with open(path, 'rb') as fh:
        head = fh.read(4096)
    if b'format ascii' in head.split(b'end_header')[0]:
        return read_ply_ascii(path)
    from ..chamfer import load_points
    return load_points(path)


def frustum_range(cams, image_height, image_width):
    """lines 59-81: cams fp32 torch [V,2,4,4] -> (center fp32 [3], size fp32 []) of the box around every camera's frustum corners at its near and far
    depth (cam[1,3,0] and cam[1,3,3])"""
    # The reference's corner list pairs image_height with x and image_width with y.  That is kept as written, because scale_mat must be what the
    # reference would have produced for the same scene.
    px = torch.tensor([[0, 0, 1], [image_height, 0, 1], [0, image_width, 1], [image_height, image_width, 1]], dtype=torch.float32)[:, :, None]
    world = []
    for cam in cams:
        rays = cam[1:2, :3, :3].inverse() @ px                                                     # [4,3,1], camera coordinates at depth 1
        pts = torch.cat([rays * cam[1, 3, 0], rays * cam[1, 3, 3]], 0)
        pts = torch.cat([pts, torch.ones_like(pts[:, -1:, :])], 1)
        world.append((cam[0:1].inverse() @ pts)[:, :3, 0])
    world = torch.cat(world, 0)
    lo, hi = world.min(0).values, world.max(0).values
    return (lo + hi) / 2, torch.max(hi - lo)


def points_range(vert):
    """lines 84-88: vert fp32 torch [N,3] -> (center, size) with size = the largest extent * 1.1"""
    lo, hi = vert.min(0).values, vert.max(0).values
    return (lo + hi) / 2, torch.max(hi - lo) * 1.1


def scene_cameras(cams, crop_wh, depth_wh, center, size):
    """lines 104-116: cams fp32 torch [V,2,4,4] -> what cameras_hd.npz holds: world_mat_<i> = the intrinsics at image_hd size (as a 4x4 with a unit
    corner) @ the extrinsics, scale_mat_<i> = the box's half size and centre"""
    scale = np.eye(4, dtype=np.float32)
    scale[:3, :3] *= size.item() / 2
    scale[:3, 3] = center.numpy()
    out = {}
    for i, cam in enumerate(cams):
        cam = sio.scale_camera(cam, (crop_wh[0] / depth_wh[0], crop_wh[1] / depth_wh[1]))
        K4 = torch.zeros(4, 4, dtype=cam.dtype)
        K4[:3, :3] = cam[1, :3, :3]
        K4[3, 3] = 1
        out['world_mat_%d' % i] = (K4 @ cam[0]).numpy()
        out['scale_mat_%d' % i] = scale.copy()
    return out


def _pair_of(v):
    w, h = [int(x) for x in str(v).split(',')] if not isinstance(v, (tuple, list)) else [int(x) for x in v]
    return w, h


def convert_scene(data_root, range_source='pcd', pthresh='.7,.7,0', prob_mask=False, resize='1920,1080', crop='1920,1072',
                  ext_image_path='eg/path/to/image/{:08}.jpg', ext_image_from_one=False, fused_depth=False, clean=None):
    """Writes <data_root>/imfunc4/{image_hd/%06d.png, mask_hd/%03d.png, depth/%03d.pfm, cameras_hd.npz} -> the imfunc4 directory.  Where
    range_source='fused' / 'clean' or fused_depth run fuse_depths, it reads the masked depths with its own defaults (view 10, vthresh 2).
    clean: a dict of cloud.clean_points keywords for range_source='clean'."""
    if range_source not in ('range', 'pcd', 'fused', 'clean'):
        raise ValueError("convert_scene: range_source must be 'range', 'pcd', 'fused' or 'clean', got %r" % (range_source,))
    if clean is not None and range_source != 'clean':
        raise ValueError("convert_scene: clean is for range_source='clean', got range_source=%r" % (range_source,))
    resize_w, resize_h = _pair_of(resize)
    crop_w, crop_h = _pair_of(crop)
    pair, cams64, depths_np, probs_np = load_mvs_output(data_root, probs=prob_mask)
    ids = pair['id_list']
    total_views = len(ids)
    cams = torch.from_numpy(cams64).float()
    depths = torch.from_numpy(depths_np).float().unsqueeze(1)
    d_w, d_h = depths.size()[-1], depths.size()[-2]
    pt = [float(v) for v in pthresh.split(',')] if isinstance(pthresh, str) else [float(v) for v in pthresh]
    if prob_mask:                                                                               # line 53
        probs = torch.from_numpy(probs_np).float().unsqueeze(2)
        masks = ((probs > torch.from_numpy(np.array(pt)).float().view(1, 3, 1, 1, 1)).sum(1) > 2.9).float()
    else:                                                                                       # line 55
        masks = torch.stack([torch.from_numpy(np.array(Image.open(os.path.join(data_root, '%s_mask.png' % i.zfill(8))).convert('L'))).float() / 255
                             for i in ids], dim=0).unsqueeze(1)
    depths *= masks

    def image_path(i):
        return ext_image_path.format(int(ids[i]) + 1 if ext_image_from_one else int(ids[i]))

    fused = None
    if range_source in ('fused', 'clean') or fused_depth:
        from .. import fusion as fu
        small = None
        if range_source in ('fused', 'clean'):
            small = np.stack([resize_bilinear_u8(load_image_u8(image_path(i)), d_w, d_h) for i in range(total_views)])
        fused = fu.fuse_depths(cams64, depths[:, 0], pair_indices(pair), images=small)
    if range_source == 'range':
        center, size = frustum_range(cams, depths[0].size()[-2], depths[0].size()[-1])
    elif range_source == 'pcd':
        center, size = points_range(torch.from_numpy(read_points(os.path.join(data_root, 'cut.ply'))).float())
    else:
        if len(fused) == 0:
            raise ValueError('convert_scene: the fusion kept no point, so there is no box to take')
        fu.save_points(os.path.join(data_root, 'all_torch.ply'), fused.points, fused.colors)
        if range_source == 'clean':
            from ..cloud import clean_fused
            fused = clean_fused(fused, **(clean or {}))
            fu.save_points(os.path.join(data_root, 'cut.ply'), fused.points, fused.colors)
        lo, hi = fused.bbox()
        center, size = points_range(torch.stack([lo, hi]).float().cpu())                       # fp32, as the cloud is once it is a PLY file

    out_dir = os.path.join(data_root, 'imfunc4')
    for sub in ('image_hd', 'mask_hd', 'depth'):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    masks_hd = (F.interpolate(masks, size=(crop_h, crop_w), mode='bilinear', align_corners=False) > 0.5).float()   # line 93
    out_depths = fused.fused_depths.cpu().numpy() if fused_depth else depths[:, 0].numpy()
    for i in range(total_views):
        img = center_crop(resize_bilinear_u8(load_image_u8(image_path(i)), resize_w, resize_h), crop_w, crop_h)
        Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(out_dir, 'image_hd', '%06d.png' % i))
        Image.fromarray(masks_hd[i, 0].numpy().astype(np.uint8) * 255).save(os.path.join(out_dir, 'mask_hd', '%03d.png' % i))
        sio.write_pfm(os.path.join(out_dir, 'depth', '%03d.pfm' % i), np.ascontiguousarray(out_depths[i]))
    np.savez(os.path.join(out_dir, 'cameras_hd.npz'), **scene_cameras(cams, (crop_w, crop_h), (d_w, d_h), center, size))
    return out_dir
