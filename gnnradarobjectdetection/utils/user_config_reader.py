from radargnn_amd.config_reader import ConfigToDataClassMapping, UserConfigurationReader, dataclass_from_dict  # noqa: F401
