"""Scene file readers of the reference with numpy / PIL only (no OpenCV, imageio or scikit-image):

* load_pfm / write_pfm, load_cam, load_pair, scale_camera: reference code/utils/my_utils.py:32-63, 334-496 (same values, same layouts);
* load_rgb / load_mask: rend_util.py:8-23 (imageio + skimage there): rgb = 2 (img / max) - 1 as [3,H,W] fp32, max = 255 or 65535 by bit depth;
  mask = grey > 127.5 with grey = PIL's 'F' conversion in 0..255 (what imageio's as_gray read returns);
* load_K_Rt_from_P: rend_util.py:25-45 with cv2.decomposeProjectionMatrix replaced by a numpy RQ decomposition: P[:, :3] = K R with K upper
  triangular with a positive diagonal and R a rotation (P's sign flipped first where det P[:, :3] < 0, P being defined up to scale), K / K[2,2],
  pose = [R^T | camera centre];
* glob_imgs: general.py:17-21.
"""
import os
import re
import sys
from glob import glob

import numpy as np
import torch
from PIL import Image


def glob_imgs(path):
    imgs = []
    for ext in ['*.png', '*.jpg', '*.JPEG', '*.JPG']:
        imgs.extend(glob(os.path.join(path, ext)))
    return imgs


def load_rgb(path):
    """-> fp32 [3,H,W] in [-1, 1]."""
    with Image.open(path) as im:
        img = np.asarray(im if im.mode in ('RGB', 'I;16') else im.convert('RGB'))
    imax = 65535.0 if img.dtype == np.uint16 else 255.0
    img = np.multiply(img, 1.0 / imax).astype(np.float32)
    if img.ndim == 2:
        img = np.repeat(img[..., None], 3, axis=2)
    img -= 0.5
    img *= 2.
    return img.transpose(2, 0, 1)


def load_mask(path):
    """-> bool [H,W]: grey value > 127.5."""
    with Image.open(path) as im:
        if im.mode in ('RGBA', 'LA', 'P', 'PA', 'CMYK', 'YCbCr'):
            im = im.convert('RGB')
        alpha = np.asarray(im.convert('F'), dtype=np.float32)
    return alpha > 127.5


def load_pfm(file):
    """-> float32 [H,W] or [H,W,3], rows bottom-up in the file flipped to top-down (a view with a negative stride, as the reference returns)."""
    with open(file, 'rb') as f:
        header = f.readline().rstrip()
        if header not in (b'PF', b'Pf'):
            raise Exception('Not a PFM file.')
        color = header == b'PF'
        dims = re.match(br'^(\d+)\s(\d+)\s$', f.readline())
        if not dims:
            raise Exception('Malformed PFM header.')
        width, height = map(int, dims.groups())
        scale = float(f.readline().rstrip())
        endian = '<' if scale < 0 else '>'
        data = np.fromfile(f, endian + 'f')
    data = np.reshape(data, (height, width, 3) if color else (height, width))
    return data[::-1, ...]


def write_pfm(file, image, scale=1):
    if image.dtype.name != 'float32':
        raise Exception('Image dtype must be float32.')
    image = np.flipud(image)
    if image.ndim == 3 and image.shape[2] == 3:
        color = True
    elif image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1):
        color = False
    else:
        raise Exception('Image must have H x W x 3, H x W x 1 or H x W dimensions.')
    endian = image.dtype.byteorder
    if endian == '<' or (endian == '=' and sys.byteorder == 'little'):
        scale = -scale
    with open(file, 'wb') as f:
        f.write(b'PF\n' if color else b'Pf\n')
        f.write(b'%d %d\n' % (image.shape[1], image.shape[0]))
        f.write(b'%f\n' % scale)
        image.tofile(f)


def load_cam(file, max_d, interval_scale=1, override=False):
    """MVSNet camera text -> float64 [2,4,4]: [0] extrinsic, [1][:3,:3] intrinsic, [1][3] = depth min, interval, count, max."""
    cam = np.zeros((2, 4, 4))
    with open(file) as f:
        words = f.read().split()
    for i in range(4):
        for j in range(4):
            cam[0][i][j] = words[4 * i + j + 1]
    for i in range(3):
        for j in range(3):
            cam[1][i][j] = words[3 * i + j + 18]
    d = cam[1][3]
    if len(words) == 29:
        d[0], d[1], d[2] = words[27], float(words[28]) * interval_scale, max_d
        d[3] = d[0] + d[1] * (d[2] - 1)
    elif len(words) == 30:
        d[0], d[1], d[2] = words[27], float(words[28]) * interval_scale, words[29]
        d[3] = d[0] + d[1] * (d[2] - 1)
    elif len(words) == 31:
        if override:
            d[0], d[1], d[2], d[3] = words[27], (float(words[30]) - float(words[27])) / (max_d - 1), max_d, words[30]
        else:
            d[0], d[1], d[2], d[3] = words[27], float(words[28]) * interval_scale, words[29], words[30]
    return cam


def load_pair(file, min_views=None):
    """pair.txt -> {id: {'id', 'index', 'pair': [source ids], 'score': [floats]}, 'id_list': [ids]}."""
    with open(file) as f:
        lines = f.readlines()
    n_cam = int(lines[0])
    pairs, img_ids = {}, []
    for i in range(1, 1 + 2 * n_cam, 2):
        img_id = lines[i].strip()
        toks = lines[i + 1].strip().split(' ')
        n_pair = int(toks[0])
        if min_views is not None and n_pair < min_views:
            continue
        pair = [toks[j] for j in range(1, 1 + 2 * n_pair, 2)]
        score = [float(toks[j + 1]) for j in range(1, 1 + 2 * n_pair, 2)]
        img_ids.append(img_id)
        pairs[img_id] = {'id': img_id, 'index': i // 2, 'pair': pair, 'score': score}
    pairs['id_list'] = img_ids
    return pairs


def scale_camera(cam, scale=1):
    """Focal lengths and principal point of cam[..., 1] scaled by scale (a number or an (x, y) tuple); numpy or torch."""
    if type(scale) != tuple:
        scale = (scale, scale)
    if isinstance(cam, np.ndarray):
        new = np.copy(cam)
    elif isinstance(cam, torch.Tensor):
        new = cam.clone()
    else:
        raise TypeError
    new[..., 1, 0, 0] = cam[..., 1, 0, 0] * scale[0]
    new[..., 1, 1, 1] = cam[..., 1, 1, 1] * scale[1]
    new[..., 1, 0, 2] = cam[..., 1, 0, 2] * scale[0]
    new[..., 1, 1, 2] = cam[..., 1, 1, 2] * scale[1]
    return new


def _rq3(M):
    """M = K R, K upper triangular with a positive diagonal, R orthonormal."""
    Q, U = np.linalg.qr(np.flipud(M).T)
    K = np.flipud(np.fliplr(U.T))
    R = np.flipud(Q.T)
    D = np.diag(np.sign(np.diag(K)))
    return K @ D, D @ R


def load_K_Rt_from_P(filename, P=None):
    """-> intrinsics float64 [4,4] (K / K[2,2]), pose float32 [4,4] (camera to world: R^T and the camera centre)."""
    if P is None:
        lines = open(filename).read().splitlines()
        if len(lines) == 4:
            lines = lines[1:]
        lines = [[x[0], x[1], x[2], x[3]] for x in (x.split(" ") for x in lines)]
        P = np.asarray(lines).astype(np.float32).squeeze()
    P = np.asarray(P, dtype=np.float64)[:3, :4]
    if np.linalg.det(P[:, :3]) < 0:
        P = -P
    K, R = _rq3(P[:, :3])
    centre = -np.linalg.solve(P[:, :3], P[:, 3])
    intrinsics = np.eye(4)
    intrinsics[:3, :3] = K / K[2, 2]
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R.transpose()
    pose[:3, 3] = centre
    return intrinsics, pose
