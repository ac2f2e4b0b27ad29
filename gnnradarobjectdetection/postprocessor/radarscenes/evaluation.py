from radargnn_amd.metrics import RadarscenesEvaluator  # noqa: F401
