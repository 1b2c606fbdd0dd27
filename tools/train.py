"""Train MVSDF on one scene: the reference's training/exp_runner.py command on this project (mvsdf_amd/training.py states the differences).

    python tools/train.py --data_dir DTU/scan24 --conf confs/mvsdf_dtu.conf --expname scan24 --exps_root . [--seed 0] [--feat_ckpt vismvsnet.pt]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mvsdf_amd import training  # noqa: E402

if __name__ == '__main__':
    torch.set_num_threads(1)                                     # idr_train.py:20
    training.main()
