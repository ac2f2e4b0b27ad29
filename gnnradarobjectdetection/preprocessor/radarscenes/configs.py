from radargnn_amd.preprocessor import RadarScenesDatasetConfiguration  # noqa: F401
