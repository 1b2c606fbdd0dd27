"""Full-image rendering + PSNR with the reference's eval loop semantics (reference code/evaluation/eval.py:127-185, 239-246;
code/training/idr_train.py:221-230): the image is split into pixel chunks (utils.general.split_input), every chunk goes through
IDRNetwork.forward in eval mode (HIP tracer in its eval branch, analytic normals: no autograd graph, unlike the reference whose normals
need autograd.grad and therefore run outside no_grad), the `rgb_values` are merged back."""
import math
import os

import numpy as np
import torch

from .utils import general as utils
from .utils.plots import lin2img


@torch.no_grad()
def render_image(model, model_input, total_pixels, n_pixels=10000):
    """-> rgb_values [B * total_pixels, 3] in [-1, 1] (1 where no surface was hit, idr.py:302).  eval.py:143-156."""
    was_training = model.training
    model.eval()
    res = []
    for s in utils.split_input(model_input, total_pixels, n_pixels=n_pixels):
        out = model(s)
        res.append({'rgb_values': out['rgb_values'].detach()})
    model.train(was_training)
    batch_size = model_input['uv'].shape[0]
    return utils.merge_output(res, total_pixels, batch_size)['rgb_values']


def calculate_psnr(img1, img2, mask):
    """eval.py:239-246: images in [0, 1]; the mean squared error is taken over the masked pixels only."""
    img1 = np.asarray(img1, dtype=np.float64)
    img2 = np.asarray(img2, dtype=np.float64)
    mse = np.mean((img1 - img2) ** 2) * (img2.shape[0] * img2.shape[1]) / mask.sum()
    if mse == 0:
        return float('inf')
    return 20 * math.log10(1.0 / math.sqrt(mse))


def evaluate_rendering(model, batches, img_res, n_pixels=10000):
    """eval.py:133-185 without the PNG / file output: `batches` yields (model_input, ground_truth) of ONE full image each
    (uv [1, H*W, 2], object_mask [1, H*W], rgb [1, H*W, 3]); -> (list of PSNRs, list of rendered images [H, W, 3] in [0, 1])."""
    total_pixels = img_res[0] * img_res[1]
    psnrs, images = [], []
    for model_input, ground_truth in batches:
        rgb_eval = render_image(model, model_input, total_pixels, n_pixels).reshape(1, total_pixels, 3)
        rgb_eval = (rgb_eval + 1.0) / 2.0
        rgb_eval = lin2img(rgb_eval, img_res).cpu().numpy()[0].transpose(1, 2, 0)
        rgb_gt = (ground_truth['rgb'].reshape(1, total_pixels, 3) + 1.0) / 2.0
        rgb_gt = lin2img(rgb_gt, img_res).cpu().numpy()[0].transpose(1, 2, 0)
        mask = lin2img(model_input['object_mask'].reshape(1, total_pixels, 1).float(), img_res).cpu().numpy()[0].transpose(1, 2, 0)
        psnrs.append(calculate_psnr(rgb_eval * mask, rgb_gt * mask, mask))
        images.append(rgb_eval)
    return psnrs, images


def extract_world_mesh(model, scale_mat, resolution=512, path=None, epoch=None, sparse=False, block=None, margin=None):
    """eval.py:109-125 with eval_cameras off: the SDF mesh on the device (mesh.surface_mesh), moved to world coordinates by scale_mat, reduced to its
    largest connected component; with `path`, written as <path>/surface_world_coordinates_<epoch>.obj.  -> the Mesh, or None if no surface.
    sparse=True: the mesh from mesh.sparse_marching_cubes (blocks of `block`^3 cells, `margin`; None: mesh.SPARSE_BLOCK / SPARSE_MARGIN)."""
    from . import mesh as M
    mesh = M.surface_mesh(model, resolution, sparse=sparse, block=M.SPARSE_BLOCK if block is None else block,
                          margin=M.SPARSE_MARGIN if margin is None else margin)
    if mesh is None:
        return None
    mesh = mesh.apply_transform(scale_mat).largest_component()
    if path is not None:
        mesh.export(os.path.join(path, 'surface_world_coordinates_{0}.obj'.format(epoch)))
    return mesh


def write_simplified_mesh(mesh, path, epoch, cell=None, target_faces=None):
    """Mesh.simplify(cell=... | target_faces=...) of the world mesh, written as <path>/surface_world_coordinates_<epoch>_simplified.obj
    -> the simplified Mesh, or None (and no file) when no face survives."""
    out = mesh.simplify(cell=cell, target_faces=target_faces)
    if out is not None:
        out.export(os.path.join(path, 'surface_world_coordinates_{0}_simplified.obj'.format(epoch)))
    return out


def evaluate(data_dir, conf, expname, exps_folder_name='exps', evals_folder_name='evals', timestamp='latest', checkpoint='latest', resolution=512,
             eval_rendering=False, exps_root='../', feat_ckpt=None, printer=print, sparse_mesh=False, mesh_block=None, mesh_margin=None,
             color_mesh=False, simplify_cell=None, simplify_faces=None, texture_mesh=False, level_seams=False, charts=False,
             chart_pad=None, min_chart_faces=None):
    """The testing command (eval.py:19-185, eval_cameras off): the model of <exps_root>/<exps_folder>/<train.expname>_<expname>/<timestamp>/checkpoints
    -> <exps_root>/<evals_folder>/<train.expname>_<expname>/surface_world_coordinates_<epoch>.obj (extract_world_mesh) and, with eval_rendering, every
    view rendered with its perfect mask as the object mask (eval.py:137) to rendering/eval_<idx:03>.png plus psnr.txt with the reference's line.
    sparse_mesh / mesh_block / mesh_margin: extract_world_mesh's sparse / block / margin.  color_mesh: besides the OBJ (written as without it), the same
    mesh in the colours of the input photographs as surface_world_coordinates_<epoch>_color.ply (raster.color_mesh_from_scene: image_hd/, the
    world_mat_i of cameras_hd.npz at pixel_center 0, visibility masked by mask_hd/).  -> {'epoch', 'evaldir', 'mesh', 'psnrs'} (+ 'color_mesh', the
    coloured Mesh or None, with color_mesh).  simplify_cell / simplify_faces (one of them): besides the OBJ (written as
    without them), write_simplified_mesh's surface_world_coordinates_<epoch>_simplified.obj; the result gets 'simplified_mesh'.  texture_mesh:
    also surface_world_coordinates_<epoch>_textured.{obj,mtl,png}, texture.texture_mesh_from_scene of the simplified mesh when a simplify option is
    given, else of the world mesh; the result gets 'textured_mesh' (the TexturedMesh, or None without a mesh); level_seams (with texture_mesh):
    its colours levelled across the label boundaries (seams.level_atlas); charts (with texture_mesh): the atlas of charts (charts.build_chart_atlas) with
    chart_pad texels of margin and charts of fewer than min_chart_faces faces absorbed (None: that module's defaults)."""
    from PIL import Image
    from .checkpoint import MODEL_SUBDIR
    from .datasets.device_batches import DeviceBatches
    from .datasets.scene_dataset import SceneDataset
    from .model.implicit_differentiable_renderer import IDRNetwork
    from .utils.config import load_conf
    torch.set_default_dtype(torch.float32)
    conf = load_conf(conf)
    expname = conf.get_string('train.expname') + '_' + expname
    expdir = os.path.join(exps_root, exps_folder_name, expname)
    if timestamp == 'latest':
        timestamps = os.listdir(expdir) if os.path.exists(expdir) else []
        if not timestamps:
            raise FileNotFoundError('WRONG EXP FOLDER: no run under %s' % expdir)
        timestamp = sorted(timestamps)[-1]
    evaldir = os.path.join(exps_root, evals_folder_name, expname)
    os.makedirs(evaldir, exist_ok=True)

    model = IDRNetwork(conf=conf.get_config('model')).cuda()
    dataset_conf = dict(conf.get_config('dataset')) if 'dataset' in conf else {}
    if feat_ckpt is not None:
        dataset_conf['feat_ckpt'] = feat_ckpt
    dataset = SceneDataset(data_dir, False, **dataset_conf)
    if eval_rendering and not hasattr(dataset, 'perfect_masks'):
        raise ValueError('--eval_rendering needs the perfect masks of the scene (%s/pmask/): the PSNR is taken inside them (eval.py:137)' % data_dir)
    scale_mat = dataset.get_scale_mat()
    saved = torch.load(os.path.join(expdir, timestamp, 'checkpoints', MODEL_SUBDIR, str(checkpoint) + '.pth'), map_location='cuda')
    model.load_state_dict(saved['model_state_dict'])
    epoch = saved['epoch']
    printer('evaluating...')
    model.eval()
    mesh = extract_world_mesh(model, scale_mat, resolution, path=evaldir, epoch=epoch, sparse=sparse_mesh, block=mesh_block, margin=mesh_margin)
    colored = None
    if color_mesh and mesh is not None:
        from . import raster
        colored = raster.color_mesh_from_scene(mesh, data_dir)
        colored.export(os.path.join(evaldir, 'surface_world_coordinates_{0}_color.ply'.format(epoch)))
    simplify = simplify_cell is not None or simplify_faces is not None
    simplified = None
    if simplify and mesh is not None:
        simplified = write_simplified_mesh(mesh, evaldir, epoch, cell=simplify_cell, target_faces=simplify_faces)
        if simplified is not None:
            printer('simplified: %d -> %d faces (cell %.6g)' % (len(mesh), len(simplified), mesh.simplify_stats['cell'] or 0.0))
    textured = None
    if texture_mesh and (simplified if simplify else mesh) is not None:
        from . import texture
        kw = dict(level_seams=True) if level_seams else {}
        if charts:
            opts = {} if chart_pad is None else dict(pad=chart_pad)
            kw.update(charts=True, chart_options=dict(opts, **({} if min_chart_faces is None else dict(min_faces=min_chart_faces))))
        textured = texture.texture_mesh_from_scene(simplified if simplify else mesh, data_dir, **kw)
        textured.export(os.path.join(evaldir, 'surface_world_coordinates_{0}_textured.obj'.format(epoch)))
        printer('textured: %d faces, atlas %d x %d at %.6g texels per pixel' % (len(textured.mesh), textured.texture.shape[1], textured.texture.shape[0],
                                                                              textured.density))
    psnrs = None
    if eval_rendering:
        images_dir = os.path.join(evaldir, 'rendering')
        os.makedirs(images_dir, exist_ok=True)
        batches = DeviceBatches(dataset, 1, -1)
        psnrs = []
        for i in range(len(dataset)):
            _, model_input, ground_truth = batches.batch(torch.tensor([i]))
            model_input['object_mask'] = model_input['perfect_mask']
            p, images = evaluate_rendering(model, [(model_input, ground_truth)], dataset.img_res)
            Image.fromarray((images[0] * 255).astype(np.uint8)).save(os.path.join(images_dir, 'eval_%03d.png' % i))
            psnrs += p
        arr = np.array(psnrs).astype(np.float64)
        msg = 'RENDERING EVALUATION {2}: psnr mean = {0} ; psnr std = {1}'.format('%.2f' % arr.mean(), '%.2f' % arr.std(), expname)
        printer(msg)
        with open(os.path.join(evaldir, 'psnr.txt'), 'w') as f:
            f.write(msg + '\n')
    res = {'epoch': epoch, 'evaldir': evaldir, 'mesh': mesh, 'psnrs': psnrs}
    if color_mesh:
        res['color_mesh'] = colored
    if simplify:
        res['simplified_mesh'] = simplified
    if texture_mesh:
        res['textured_mesh'] = textured
    return res


def eval_parser():
    import argparse
    p = argparse.ArgumentParser(description='Evaluate a trained MVSDF run: world-coordinate mesh and, optionally, rendering PSNR (the reference\'s evaluation/eval.py).')
    p.add_argument('--data_dir', type=str, default='fill_in_data_dir')
    p.add_argument('--conf', type=str, default='./confs/mvsdf_dtu.conf')
    p.add_argument('--expname', type=str, default='test', help='The experiment name to be evaluated.')
    p.add_argument('--exps_folder', type=str, default='exps', help='The experiments folder name.')
    p.add_argument('--gpu', type=str, default='auto', help='GPU to use: an index, or auto / ignore (the current device)')
    p.add_argument('--timestamp', default='latest', type=str, help='The experiment timestamp to test.')
    p.add_argument('--checkpoint', default='latest', type=str, help='The trained model checkpoint to test')
    p.add_argument('--resolution', default=512, type=int, help='Grid resolution for marching cube')
    p.add_argument('--eval_rendering', default=False, action='store_true', help='If set, evaluate rendering quality.')
    p.add_argument('--exps_root', type=str, default='../', help='Directory that holds exps/ and evals/ (the reference uses ../).')
    p.add_argument('--feat_ckpt', type=str, default=None, help='Vis-MVSNet checkpoint for the feature extractor (SceneDataset feat_ckpt).')
    p.add_argument('--sparse_mesh', default=False, action='store_true',
                   help='Extract the mesh from the SDF evaluated only in blocks near the surface (the same mesh as the dense grid when every surface '
                        'component reaches a seed block; mesh.sparse_marching_cubes).')
    p.add_argument('--mesh_block', default=8, type=int, help='With --sparse_mesh: the block edge in grid cells.')
    p.add_argument('--mesh_margin', default=0.5, type=float, help='With --sparse_mesh: the Lipschitz bound assumed of the SDF when seeding blocks.')
    p.add_argument('--color_mesh', default=False, action='store_true',
                   help='Also write surface_world_coordinates_<epoch>_color.ply: the mesh in the colours of image_hd/ (mvsdf_amd/raster.py).')
    g = p.add_mutually_exclusive_group()
    g.add_argument('--simplify_cell', default=None, type=float,
                   help='Also write surface_world_coordinates_<epoch>_simplified.obj: Mesh.simplify on a grid of this edge (world units).')
    g.add_argument('--simplify_faces', default=None, type=int, help='The same with Mesh.simplify(target_faces=N): at most N faces.')
    p.add_argument('--texture_mesh', default=False, action='store_true',
                   help='Also write surface_world_coordinates_<epoch>_textured.obj / .mtl / .png: the simplified mesh (with a simplify option, else the '
                        'world mesh) with a texture atlas from image_hd/ (mvsdf_amd/texture.py).')
    p.add_argument('--level_seams', default=False, action='store_true',
                   help='With --texture_mesh: level the colours across the label boundaries of the atlas (mvsdf_amd/seams.py).')
    p.add_argument('--charts', default=False, action='store_true',
                   help='With --texture_mesh: one rectangle per connected region of a view instead of one patch per face (mvsdf_amd/charts.py).')
    p.add_argument('--chart_pad', default=None, type=int, choices=(1, 2, 4, 8), help='With --charts: margin and alignment of the rectangles in texels (default 4).')
    p.add_argument('--min_chart_faces', default=None, type=int, help='With --charts: charts of fewer faces are absorbed by their neighbours (default 4).')
    return p


def main(argv=None, printer=print):
    from .training import select_gpu
    opt = eval_parser().parse_args(argv)
    select_gpu(opt.gpu)
    return evaluate(data_dir=opt.data_dir, conf=opt.conf, expname=opt.expname, exps_folder_name=opt.exps_folder, evals_folder_name='evals',
                    timestamp=opt.timestamp, checkpoint=opt.checkpoint, resolution=opt.resolution, eval_rendering=opt.eval_rendering,
                    exps_root=opt.exps_root, feat_ckpt=opt.feat_ckpt, printer=printer, sparse_mesh=opt.sparse_mesh, mesh_block=opt.mesh_block,
                    mesh_margin=opt.mesh_margin, color_mesh=opt.color_mesh, simplify_cell=opt.simplify_cell, simplify_faces=opt.simplify_faces,
                    texture_mesh=opt.texture_mesh, level_seams=opt.level_seams, charts=opt.charts, chart_pad=opt.chart_pad,
                    min_chart_faces=opt.min_chart_faces)
