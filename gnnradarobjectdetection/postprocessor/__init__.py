from radargnn_amd.metrics import evaluation_selector  # noqa: F401
