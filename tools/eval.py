"""Evaluate a trained MVSDF run: the reference's evaluation/eval.py command on this project (mvsdf_amd/evaluation.py::evaluate).

    python tools/eval.py --data_dir DTU/scan24 --conf confs/mvsdf_dtu.conf --expname scan24 --exps_root . [--eval_rendering] [--resolution 512] [--color_mesh]
                         [--simplify_cell C | --simplify_faces N] [--texture_mesh [--level_seams] [--charts [--chart_pad P] [--min_chart_faces N]]]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mvsdf_amd import evaluation  # noqa: E402

if __name__ == '__main__':
    evaluation.main()
