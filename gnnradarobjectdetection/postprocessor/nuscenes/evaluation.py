from radargnn_amd.nuscenes_eval import NuscenesEvaluator, get_submission  # noqa: F401
