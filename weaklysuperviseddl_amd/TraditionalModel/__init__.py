"""Drop-in surfaces mirroring the reference's ``TraditionalModel/`` modules (same public names)."""
from .ClassificationModel import FrozenResNetCAM, train_fc_only, evaluate_classification  # noqa: F401
from .LayerCAM import LayerCAMGenerator, CAMGenerator, evaluate_layercam_on_test_set, sweep_cam_thresholds  # noqa: F401
from .PsuedoMasks import (generate_pseudo_masks, keep_largest, generate, stage_handoff, generate_prototype_pseudo_masks,  # noqa: F401
                          prototype_cam, generate_adaptive_pseudo_masks, generate_adaptive_prototype_pseudo_masks, adaptive_masks)
from .SegmentationModel import (SegmentationModel, build_segmentation_model, train_step, train_step_mean_teacher, evaluate_model,  # noqa: F401
                                train_segmentation_model, evaluate_boundary_iou, evaluate_surface_distances,
                                predict_multiscale, train_step_consistency, train_step_mixed, evaluate_calibration)
from .AlternatingDirectionCutLoss import (  # noqa: F401
    LocalNormalizedCutLoss, compute_affinities, refine_pseudo_mask, refine_pseudo_masks_batched, train_model,
    refine_dataset, run_alternating_training, network_soft_prediction, apply_dense_crf,
    generate_crf_pseudo_masks)
from .AlternatingDirectionBoundaryLoss import ConstrainToBoundaryLossSingle  # noqa: F401
from .ExtraUtilities import compute_iou_and_acc, download_data, load_split_data  # noqa: F401
from .AffinityNet import AffinityNet, affinity_labels_from_cam, train_affinity_net  # noqa: F401
from .BoundaryNet import BoundaryNet, train_boundary_net  # noqa: F401
from .ProjectionNet import ProjectionNet, TrunkFeatures, train_projection_net  # noqa: F401
from .SegmentationDataset import PseudoSegmentationDataset, InMemoryPseudoDataset, images_to_tensor_device  # noqa: F401
