from radargnn_amd.graph_constructor.graph import build_geometric_graph  # noqa: F401
from radargnn_amd.nuscenes import convert_bounding_boxes, convert_point_cloud  # noqa: F401
