from radargnn_amd.preprocessor import RadarPointCloud  # noqa: F401
