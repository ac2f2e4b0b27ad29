"""Architecture description consumed by ``DetNetBasic`` -- field-compatible with the reference's
``gnn/configs.py:4-30`` (``GNNArchitectureConfig``) so YAML files, JSON dumps and positional construction
(``GNNArchitectureConfig(2, 3, [5], [3], [3], conv_layer_type=...)``, test/test_gnn.py:28-39) keep working.  ``TrainingConfig``
(``gnn/configs.py:33-100``) is the hyper-parameter record of ``radargnn_amd.gnn.trainer.Trainer``: same fields, order and defaults."""
from dataclasses import dataclass, field
from typing import List, Optional


@dataclass
class GNNArchitectureConfig:
    # widths of the raw node / edge feature vectors entering the network
    node_feature_dimension: int
    edge_feature_dimension: int
    # output width of every graph-convolution layer, then the two heads (last entry = output width)
    conv_layer_dimensions: List[int]
    classification_head_layer_dimensions: List[int]
    regression_head_layer_dimensions: List[int]
    # optional embedding MLPs in front of the convolutions (last entry = embedded width)
    initial_node_feature_embedding: bool = False
    initial_edge_feature_embedding: bool = False
    node_feature_embedding_layer_dimensions: Optional[List[int]] = None
    edge_feature_embedding_layer_dimensions: Optional[List[int]] = None
    conv_layer_type: str = "MPNNConv"          # or "RadarPointGNNConv"
    # inside the MLPs / convolutions
    batch_norm_in_mlps: bool = True
    conv_pre_mlp_layer_number: int = 1
    conv_post_mlp_layer_number: int = 1
    conv_use_edge_encoder: bool = False
    aggregation_function: str = "max"          # "max" | "mean" | "add" ("sum") | "min" | "var" | "std"


# class order of the two datasets' label columns, and the weight a class gets when the configuration names none
DEFAULT_CLASS_WEIGHTS = {
    "radarscenes": (("car", 1), ("pedestrian", 1), ("pedestrian_group", 1), ("two_wheeler", 1), ("large_vehicle", 1),
                    ("background", 0.05)),
    "nuscenes": (("background", 0.05), ("barrier", 1), ("bicycle", 1), ("bus", 1), ("car", 1), ("construction", 1),
                 ("motorcycle", 1), ("pedestrian", 1), ("trafficcone", 1), ("trailer", 1), ("truck", 1)),
}


@dataclass
class TrainingConfig:
    dataset: str                               # "radarscenes" | "nuscenes"
    learning_rate: float
    epochs: int
    batch_size: int
    shuffle: bool
    bg_index: int                              # label of the background class: its nodes carry no box
    deterministic: bool = False
    seed: int = 0
    # cross-entropy weight per class, in label order (missing classes get the dataset's default)
    class_weights: dict = field(default_factory=dict)
    set_weights_according_radar_scenes_distribution: bool = False
    val_class_weights: dict = field(default_factory=dict)       # empty: the training weights
    bb_loss_weight: float = 1
    cls_loss_weight: float = 1
    regularization_strength: float = 1e-4      # Adam's weight decay (L2)
    reduce_lr_on_plateau_factor: float = 0.5
    reduce_lr_on_plateau_patience: int = 0     # > 0: ReduceLROnPlateau on the validation loss
    exponential_lr_decay_factor: float = 0.0   # else > 0: ExponentialLR; else a constant rate
    early_stopping_patience: int = 10
    adapt_orientation_angle: bool = False      # train on sin of the box angle folded into [-pi/2, pi/2]

    def __post_init__(self):
        if self.dataset not in DEFAULT_CLASS_WEIGHTS:
            raise ValueError("Only the radarscenes and nuscenes dataset are supported!")
        for name, weight in DEFAULT_CLASS_WEIGHTS[self.dataset]:
            self.class_weights.setdefault(name, weight)
        if self.val_class_weights:
            assert set(self.class_weights.keys()) == set(self.val_class_weights.keys()), \
                "class_weights and val_class_weights must name the same classes"
        else:
            self.val_class_weights = self.class_weights
