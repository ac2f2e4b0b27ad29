from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration  # noqa: F401
