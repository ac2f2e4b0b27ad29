from radargnn_amd.nuscenes import NuScenesDatasetConfiguration  # noqa: F401
