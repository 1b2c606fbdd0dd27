#!/usr/bin/env python3
"""Simplify a mesh on the GPU: vertex clustering on a uniform grid with quadric-error placement (Mesh.simplify, which states the definition):

    python tools/simplify_mesh.py IN OUT (--cell C | --faces N) [--placement quadric|mean]

Reads and writes OBJ or PLY (by extension; load_mesh / Mesh.export).  --cell is the grid's edge in the mesh's units; --faces searches for the
smallest grid that leaves at most N faces.  Prints the counts."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('in_file', type=str)
    p.add_argument('out_file', type=str)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument('--cell', type=float, default=None, help='the grid\'s edge (finite, > 0)')
    g.add_argument('--faces', type=int, default=None, help='at most this many faces')
    p.add_argument('--placement', choices=('quadric', 'mean'), default='quadric')
    args = p.parse_args(argv)
    if not os.path.exists(args.in_file):
        p.exit(1, 'simplify_mesh.py: %s: no such file\n' % args.in_file)
    from mvsdf_amd.mesh import load_mesh
    mesh = load_mesh(args.in_file).to('cuda')
    out = mesh.simplify(cell=args.cell, target_faces=args.faces, placement=args.placement)
    st = mesh.simplify_stats
    kept = 0 if out is None else len(out)
    print('[simplify] num faces from %d to %d (cell %s, %d clusters, %d vertices, %d degenerate, %d duplicates)'
          % (len(mesh), kept, st['cell'], st['clusters'], st['vertices'], st['degenerate'], st['duplicates']))
    if out is None:
        p.exit(1, 'simplify_mesh.py: no face survived; nothing written\n')
    out.export(args.out_file)


if __name__ == '__main__':
    main()
