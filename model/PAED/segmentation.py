"""Entry-point shim for the reference's model/PAED/segmentation.py (`from segmentation import compute_sdf`,
`from segmentation import CrackSeg`): the names resolve to the MI355X implementation."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from visiontransformer_amd.sdf import compute_sdf  # noqa: E402,F401
from visiontransformer_amd.skeleton import CrackSeg, skeletonize  # noqa: E402,F401
