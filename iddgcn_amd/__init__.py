"""iddgcn_amd — MI355X-native hot path of IDDGCN (AhauBioinformatics/IDDGCN).

The directed multi-relational graph convolution of prediction/IDDGCN.py,
forward and backward, as hand-written HIP kernels for gfx950 behind a C-ABI
(include/iddgcn.h, libiddgcn_hip.so), driven from a Keras-shaped Python
surface:

    from iddgcn_amd import get_IDDGCN_Model, get_adj_mats, Adam, BinaryCrossentropy
"""
from ._lib import IddgcnError  # noqa: F401
from .graph import get_adj_mats  # noqa: F401
from .model import (Adam, BinaryCrossentropy, DistMult, IDDGCN_Layer, IDDGCN_Model,  # noqa: F401
                    SaveWeightsCallback, get_IDDGCN_Model)
from .utils import generate_reverse_triplets, get_y_true  # noqa: F401
from .metrics import classification_metrics, classification_metrics_device, ranking_metrics  # noqa: F401
from . import explain  # noqa: F401,E402  (explaiNE / GNNExplainer / IDDGCN explainer on the HIP path)
from .explain import fidelity_curves, fidelity_summary, random_explanations  # noqa: F401,E402
from .explain import counterfactual_batched, counterfactual_summary, occlusion_batched  # noqa: F401,E402
from .explain import integrated_gradients_batched, integrated_gradients_summary  # noqa: F401,E402
from . import similarity  # noqa: F401,E402  (feat_similarity.py similarity graph on MFMA)
from . import ground_truth  # noqa: F401,E402  (explanation ground truth on the GPU, P/R/F1@k of the explainers)
from .ground_truth import (construct_ground_truth, evaluate_explanations, filter_ground_truth,  # noqa: F401,E402
                           ground_truth_table, load_similarity_csv)
