"""The part of the reference's ``preprocessor`` package that runs on the MI355X (radargnn_amd.preprocessor / .groundtruth /
.graph_constructor.configs): frames from a sequence's detection table, box targets, the configuration dataclasses.  The dataset
classes around them (file layout, splits, nuScenes conversion) stay with the reference."""
from .nuscenes.configs import NuScenesDatasetConfiguration as _NuScenesDatasetConfiguration
from .radarscenes.configs import RadarScenesDatasetConfiguration as _RadarScenesDatasetConfiguration

# utils/user_config_reader.py picks the dataset-processing dataclass here; ``dataset_selector`` (the dataset classes, which read the
# datasets' own files) stays with the reference
config_selector = {"radarscenes": _RadarScenesDatasetConfiguration, "nuscenes": _NuScenesDatasetConfiguration}
