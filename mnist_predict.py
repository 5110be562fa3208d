#!/usr/bin/env python3
"""Evaluate a saved checkpoint (``mnist_cnn.pt``) on the MNIST test split.

Prints the reference's ``Test set: Average loss ...`` line; small batches run the single-launch
fused MI355X inference kernel, ``--no-cuda`` the reference torch math.  See
``python mnist_predict.py --help``.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_mnist_ddp_amd.inference import predict_main  # noqa: E402

if __name__ == '__main__':
    sys.exit(predict_main())
