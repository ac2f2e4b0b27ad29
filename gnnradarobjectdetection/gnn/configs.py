from radargnn_amd.gnn.configs import GNNArchitectureConfig, TrainingConfig  # noqa: F401
