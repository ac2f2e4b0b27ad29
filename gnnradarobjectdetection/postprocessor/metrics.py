from radargnn_amd.metrics import ObjectDetectionMetrics, SegmentationMetrics  # noqa: F401
