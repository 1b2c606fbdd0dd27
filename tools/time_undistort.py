"""Device time of undistort_images (mvsdf_amd/undistort.py, csrc/undistort.hip) at a realistic load, beside torch.nn.functional.grid_sample on the same
GPU for the same map: the median of --repeats runs after a warm-up, each between two device events, one JSON line per camera model.

One camera, --views images of --width x --height x --channels uint8 on the device, all in one launch.  The effective rate counts the bytes the kernel
must read and write once (the images in, the images and the mask out) over its time.  grid_sample takes float32 planes [V, C, H, W] and a
normalised grid (built beforehand from distort_points, not timed; neither is the conversion of the images), so it moves four times the bytes and
rounds otherwise: it is compared by TIME only.

    python tools/time_undistort.py [--models SIMPLE_RADIAL,OPENCV_FISHEYE --views 64 --width 4000 --height 3000 --channels 3 --repeats 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# distortion per model at a focal length of 0.8 widths: a few percent at the corners, as a phone or action camera has
COEFFICIENTS = {'SIMPLE_RADIAL': [-0.08], 'RADIAL': [-0.08, 0.01], 'OPENCV': [-0.08, 0.01, 0.001, -0.001], 'FULL_OPENCV': [-0.08, 0.01, 0.001, -0.001, 0.002, 0.01, 0.0, 0.0],
                'OPENCV_FISHEYE': [0.03, -0.005, 0.001, 0.0], 'SIMPLE_RADIAL_FISHEYE': [0.03], 'RADIAL_FISHEYE': [0.03, -0.005], 'PINHOLE': []}
ONE_FOCAL = ('SIMPLE_RADIAL', 'RADIAL', 'SIMPLE_RADIAL_FISHEYE', 'RADIAL_FISHEYE')


def make_camera(model, W, H):
    f = 0.8 * W
    return {'model': model, 'width': W, 'height': H, 'params': np.array(([f] if model in ONE_FOCAL else [f, f]) + [W / 2 + 3.3, H / 2 - 2.1] + COEFFICIENTS[model])}


def timed(fn, repeats):
    fn()                                                                    # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return out, ms


def grid_for(camera, out_camera, undistort):
    """the normalised sampling grid [1, H', W', 2] of grid_sample (align_corners=False) for the same source coordinates"""
    Wo, Ho = out_camera['width'], out_camera['height']
    y, x = torch.meshgrid(torch.arange(Ho, dtype=torch.float64, device='cuda') + 0.5, torch.arange(Wo, dtype=torch.float64, device='cuda') + 0.5, indexing='ij')
    src = undistort.distort_points(torch.stack([x.reshape(-1), y.reshape(-1)], 1), camera, out_camera)
    g = torch.stack([src[:, 0] / camera['width'] * 2 - 1, src[:, 1] / camera['height'] * 2 - 1], 1)
    return g.reshape(1, Ho, Wo, 2).to(torch.float32)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--models', type=str, default='SIMPLE_RADIAL,OPENCV_FISHEYE')
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--width', type=int, default=4000)
    ap.add_argument('--height', type=int, default=3000)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no_torch', action='store_true', help='time the kernel alone')
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    assert torch.cuda.is_available(), 'time_undistort.py measures on the GPU'
    from mvsdf_amd import undistort
    V, W, H, C = a.views, a.width, a.height, a.channels
    g = torch.Generator(device='cuda').manual_seed(0)
    images = torch.randint(0, 256, (V, H, W, C), dtype=torch.uint8, device='cuda', generator=g)
    results = []
    for model in a.models.split(','):
        cam = make_camera(model, W, H)
        out_cam = undistort.undistorted_camera(cam)
        Wo, Ho = out_cam['width'], out_cam['height']
        (out, mask), k_ms = timed(lambda: undistort.undistort_images(images, cam, out_cam), a.repeats)
        moved = V * H * W * C + V * Ho * Wo * C + Ho * Wo
        med = float(np.median(k_ms))
        res = {'model': model, 'views': V, 'source': [W, H, C], 'output': [Wo, Ho], 'repeats': a.repeats, 'kernel_ms': round(med, 3),
               'kernel_runs': [round(v, 3) for v in k_ms], 'bytes_moved': moved, 'effective_GBps': round(moved / med * 1e-6, 1),
               'valid_fraction': round(float(mask.float().mean()), 4)}
        del out
        if not a.no_torch:
            grid = grid_for(cam, out_cam, undistort)
            planes = images.permute(0, 3, 1, 2).float().contiguous()
            dst = torch.empty(V, C, Ho, Wo, dtype=torch.float32, device='cuda')

            def by_torch():
                for v in range(V):
                    dst[v:v + 1] = torch.nn.functional.grid_sample(planes[v:v + 1], grid, mode='bilinear', padding_mode='border', align_corners=False)
                return dst
            _, t_ms = timed(by_torch, a.repeats)
            res.update({'grid_sample_ms': round(float(np.median(t_ms)), 3), 'grid_sample_runs': [round(v, 3) for v in t_ms],
                        'grid_sample_over_kernel': round(float(np.median(t_ms)) / med, 2)})
            del planes, dst, grid
        print(json.dumps(res), flush=True)
        results.append(res)
    return results


if __name__ == '__main__':
    main()
