from radargnn_amd.postprocessor import BoxSuppressor, GroundTruthExtractor, Postprocessor, PredictionExtractor  # noqa: F401
