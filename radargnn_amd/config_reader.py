"""The user configuration file of the reference's scripts (utils/user_config_reader.py; configurations/*.yml) read into the
configuration dataclasses this package mirrors.

A file has three super-tasks -- ``CREATE_DATASET`` (with the ``dataset`` name, ``DATASET_PROCESSING`` and ``GRAPH_CONSTRUCTION``),
``TRAIN`` (``MODEL_ARCHITECTURE``, ``TRAINING``) and ``EVALUATE`` (``POSTPROCESSING``) -- and every subset becomes one dataclass
instance: ``UserConfigurationReader.get_config_object("TRAINING", UserConfigurationReader.read_config_file(path))``."""
from __future__ import annotations

import dataclasses

import yaml

from .gnn.configs import GNNArchitectureConfig, TrainingConfig
from .graph_constructor.configs import GraphConstructionConfiguration
from .nuscenes import NuScenesDatasetConfiguration
from .postprocessor import PostProcessingConfiguration
from .preprocessor import RadarScenesDatasetConfiguration

# the dataset-processing dataclass of each dataset (the reference's ``preprocessor.config_selector``)
config_selector = {"radarscenes": RadarScenesDatasetConfiguration, "nuscenes": NuScenesDatasetConfiguration}


def dataclass_from_dict(data_class, d):
    """``d`` as an instance of ``data_class``, fields that are dataclasses themselves converted in turn.  Whatever cannot be
    converted -- ``data_class`` is no dataclass (``dict``, ``List[int]``, ...), a key it has no field for, a constructor that
    refuses the values -- is returned as it came: the caller tells success by the type of the result."""
    if not (dataclasses.is_dataclass(data_class) and isinstance(d, dict)):
        return d
    field_types = {f.name: f.type for f in dataclasses.fields(data_class)}
    if any(key not in field_types for key in d):
        return d
    try:
        return data_class(**{key: dataclass_from_dict(field_types[key], value) for key, value in d.items()})
    except Exception:
        return d


class ConfigToDataClassMapping:

    @staticmethod
    def get_mapping_dicts(dataset: str):
        """-> ({subset name: dataclass}, {subset name: the super-task it sits under})."""
        dataclass_mapping_dict = {"DATASET_PROCESSING": config_selector[dataset],
                                  "GRAPH_CONSTRUCTION": GraphConstructionConfiguration,
                                  "MODEL_ARCHITECTURE": GNNArchitectureConfig,
                                  "TRAINING": TrainingConfig,
                                  "POSTPROCESSING": PostProcessingConfiguration}
        supertask_mapping_dict = {"DATASET_PROCESSING": "CREATE_DATASET",
                                  "GRAPH_CONSTRUCTION": "CREATE_DATASET",
                                  "MODEL_ARCHITECTURE": "TRAIN",
                                  "TRAINING": "TRAIN",
                                  "POSTPROCESSING": "EVALUATE"}
        return dataclass_mapping_dict, supertask_mapping_dict


class UserConfigurationReader:

    @staticmethod
    def get_config_object(config_subset_name: str, config_dict: dict):
        """The subset ``config_subset_name`` of a configuration read by ``read_config_file`` as its dataclass instance."""
        dataset = config_dict["CREATE_DATASET"]["dataset"]
        classes, super_tasks = ConfigToDataClassMapping.get_mapping_dicts(dataset)
        wanted = classes.get(config_subset_name)
        subset = config_dict.get(super_tasks.get(config_subset_name)).get(config_subset_name)
        config = dataclass_from_dict(wanted, subset)
        if wanted is None or not isinstance(config, wanted):
            raise Exception("Conversion of config file to dataclass failed.")
        return config

    @staticmethod
    def read_config_file(path: str):
        with open(path) as f:
            return yaml.safe_load(f)
