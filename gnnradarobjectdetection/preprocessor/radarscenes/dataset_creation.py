from radargnn_amd.data import create_graph_data  # noqa: F401
from radargnn_amd.groundtruth import GroundTruthCreator  # noqa: F401
from radargnn_amd.preprocessor import (PointCloudProcessor, SequenceTable, create_graph_data_from_sequence,  # noqa: F401
                                       create_point_cloud_frames)
