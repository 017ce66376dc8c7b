"""wats_hip -- MI355X-native graph-wavelet feature extractor (WATS hot path).

Drop-in for the hot path of ``calibration/WATS.py`` (CaptainCuong/Efficient-GNN):
the Chebyshev-polynomial heat-kernel wavelet features computed by hand-written
gfx950 HIP kernels behind a C ABI (``include/wats_hip.h``).

Public surface (reference names):
    compute_normalized_laplacian (-> SymNormalizedLaplacian, L_sym with the
    reference's `(2/2.0)*L - identity(N)` arithmetic), chebyshev_polynomials
    (applies its operator literally), graph_wavelet_features,
    WATS  (calibrator), NormalizedLaplacian (device L_hat handle).
Section 8(f): SparseCompatibleGCN / RowNormalizedAdjacency (the base model's
propagation as a HIP SpMM), EdgeProbe / target_flip_scores / toggle_edges
(its gradient at edge positions and the attack's flip, HIP SDDMM),
RowNormalizedAdjacency.with_flips / FlippedAdjacency (a flipped graph as a view
of its parent's operators, committed to CSR without a rebuild), edge_index_to_csr / DeviceCSR (edge_index to canonical CSR on the device), metrics
(device ECE), GATSCalibrator / GATS / CalibAttentionLayer / shortest_path_length (the
comparison calibrator of the harness: its edge softmax, both aggregations and its BFS in HIP,
edge_softmax_attention on an AttentionGraph), CaGCN / GCNConv / calibration_loss (the GCN-based calibrator: PyG's
gcn_norm + propagate as one HIP aggregation, sym_norm_aggregate on a SymNormGraph), SimCalib / SimilarityBank /
similarity_temperature (the similarity-based calibrator: cosine similarity, softmax and the confidence product as one
fused HIP pass per direction, no (N, N_val) matrix), DCGC / DecisiveEdge / EdgeWeightGraph / edge_mlp_weights /
weighted_propagate / homophily_weights (the edge-weight calibrator: its edge MLP as one fused pass per direction on the
float32 matrix cores with no (E, k) tensor, and the base model's propagation with the edge values as an argument),
GETSCalibrator / GCNExpert / gated_sym_norm_head / calibrate_with_gets (the mixture-of-graph-experts calibrator: the
last propagation of every expert, the top-k gated mixture, softplus and log_softmax as one HIP pass that reads only
the selected slices, no (N, E, C) tensor of aggregated outputs), Calib_FGA / flip_select / target_logits (the
reference's calibration attack as a drop-in class on the sparse path: the flip selection in one HIP pass and the
candidate's logits from the 2-hop ball of the target; Calib_FGA.attack_many / fga_scores run many targets in lock
step with the gradient's row and column in closed form, one HIP pass over z and h for all of them), Calib_IGA / iga_path_logits / iga_scores (the reference's
integrated-gradients attack: its path integrals in closed form, all targets scored in one HIP pass over z and h),
Calib_Random / Calib_RND / trial_logits (the reference's random baseline attacks: a step's trials drawn ahead from
the reference's own random stream and evaluated by one HIP launch, several targets in lock step),
TemperatureScaling / VectorScaling / MatrixScaling / ETS / scaled_log_probs / train_scaling (the node-wise calibrators:
their row maps fused in HIP, a training epoch -- loss, gradients, Adam, early stopping -- in one launch on a device
state block; train_wats_head and WATS(fused_training=True): the same for WATS's temperature head), calibration_report / CalibrationReport / evaluate_calibration / evaluate_calibration_probs /
reliability_curves / average_ece_many (the harness's evaluation step: accuracy, confidence, per-class and top-label
ECE, NLL, Brier and the reliability curves from one fused HIP binning pass and one host read).
"""
from ._lib import LIB_PATH, WaveletError  # noqa: F401
from .graphgen import CSRGraph, named_graph, rmat_graph  # noqa: F401
from .laplacian import NormalizedLaplacian, dense_to_csr  # noqa: F401
from .wavelet import (  # noqa: F401
    SymNormalizedLaplacian,
    as_laplacian,
    as_operator,
    chebyshev_polynomials,
    compute_normalized_laplacian,
    graph_wavelet_features,
    heat_coefficients,
    row_l1_normalize,
)
from .WATS import WATS, accuracy  # noqa: F401
from .gcn import (  # noqa: F401
    EdgeProbe,
    RowNormalizedAdjacency,
    SparseCompatibleGCN,
    propagate,
    rowdot,
    sddmm,
    target_flip_scores,
    target_scores_from_grad,
    toggle_edges,
)
from .head import train_wats_head, wats_head  # noqa: F401
from .ingest import DeviceCSR, edge_index_to_csr  # noqa: F401
from .flips import FlippedAdjacency  # noqa: F401
from .attack import (  # noqa: F401
    Calib_FGA,
    Calib_IGA,
    Calib_Random,
    Calib_RND,
    fga_scores,
    fga_scores_workspace,
    flip_select,
    iga_path_logits,
    iga_scores,
    kl_divergence_target,
    kl_divergence_with_uniform,
    overconfidence_objective,
    target_logits,
    trial_logits,
    underconfidence_objective,
)
from .gats import (  # noqa: F401
    GATS,
    AttentionGraph,
    CalibAttentionLayer,
    GATSCalibrator,
    calibrate_with_gats,
    csr_transpose_map,
    edge_softmax_attention,
    shortest_path_length,
)
from .cagcn import (  # noqa: F401
    CaGCN,
    GCNConv,
    SymNormGraph,
    calibration_loss,
    sym_norm_aggregate,
)
from .simcalib import (  # noqa: F401
    SimCalib,
    SimilarityBank,
    raw_similarity_temperature,
    similarity_temperature,
)
from .dcgc import (  # noqa: F401
    DCGC,
    DecisiveEdge,
    EdgeWeightGraph,
    edge_mlp_weights,
    homophily_weights,
    weighted_propagate,
)
from .gets import (  # noqa: F401
    GCNExpert,
    GETSCalibrator,
    calibrate_with_gets,
    gated_sym_norm_head,
)
from .scaling import (  # noqa: F401
    ETS,
    MS,
    TS,
    VS,
    MatrixScaling,
    TemperatureScaling,
    VectorScaling,
    calibrate_with_matrix_scaling,
    calibrate_with_temperature_scaling,
    calibrate_with_vector_scaling,
    ensemble_weights,
    ets_label_probs,
    scaled_log_probs,
    train_scaling,
)
from .metrics import (  # noqa: F401
    CalibrationReport,
    average_ece_many,
    calculate_average_ece,
    calculate_ece,
    calibration_report,
    evaluate_calibration,
    evaluate_calibration_probs,
    reliability_curves,
)

__version__ = "0.1.0"
