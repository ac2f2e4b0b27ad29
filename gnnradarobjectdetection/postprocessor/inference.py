from radargnn_amd.inference import Predictor  # noqa: F401
