"""The part of the reference's ``preprocessor`` package that runs on the MI355X (radargnn_amd.preprocessor / .groundtruth /
.graph_constructor.configs): frames from a sequence's detection table, box targets, the configuration dataclasses.  The dataset
classes around them (file layout, splits, nuScenes conversion) stay with the reference."""
