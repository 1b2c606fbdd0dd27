#!/usr/bin/env python3
"""Trim a mesh on the GPU, like the reference's code/mesh_cut/mesh_cut.py:

    python tools/mesh_cut.py IN_OBJ OUT_OBJ [--thresh 15] [--smooth 10]

Reads what Mesh.export writes (OBJ / PLY with vertex colours (1 - s, s, 0)), removes the faces of the minimum cut (Mesh.trim: S*, the faces
reachable from the source after a maximum flow) and the vertices only they used, and writes OUT (format by extension).  Prints the reference's
'[trim] num faces from F to F'' line."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('in_file', type=str)
    p.add_argument('out_file', type=str)
    p.add_argument('--thresh', type=int, default=15, help='a face is bright (tied to the source) when its mean red > thresh / 255')
    p.add_argument('--smooth', type=int, default=10, help='capacity each half-edge adds between two faces (>= 0)')
    args = p.parse_args(argv)
    if args.smooth < 0:
        p.error('--smooth must be >= 0')
    if not os.path.exists(args.in_file):
        p.exit(1, 'mesh_cut.py: %s: no such file\n' % args.in_file)
    from mvsdf_amd.mesh import load_mesh
    mesh = load_mesh(args.in_file).to('cuda')
    out = mesh.trim(args.thresh, args.smooth)
    nf = len(mesh)
    kept = 0 if out is None else len(out)
    print(f'[trim] num faces from {nf} to {kept}')
    if out is None:
        p.exit(1, 'mesh_cut.py: every face was removed; nothing written\n')
    out.export(args.out_file)


if __name__ == '__main__':
    main()
