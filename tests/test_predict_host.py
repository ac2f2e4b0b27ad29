"""Host side of the inference driver (radargnn_amd/inference.py, radargnn_amd/config_reader.py) and of the import-path shim: the
grouping of loader batches into steps, every import of the reference's ``evaluate.py`` and ``train.py``, and the two shipped
configuration files (copies under tests/golden/) read into the five configuration objects.  No GPU."""
import copy
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUBSETS = ("DATASET_PROCESSING", "GRAPH_CONSTRUCTION", "MODEL_ARCHITECTURE", "TRAINING", "POSTPROCESSING")


def test_plan_steps_groups_whole_loader_batches():
    from radargnn_amd.inference import plan_steps
    assert plan_steps([1] * 7, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert plan_steps([5, 5, 2], 4) == [[0], [1], [2]]                # a batch larger than the step size: a step of its own
    assert plan_steps([2, 2, 2], 3) == [[0, 1], [2]]                  # never split: the first step holds 4 graphs
    assert plan_steps([], 8) == []
    assert plan_steps([1] * 5, 100) == [[0, 1, 2, 3, 4]]
    with pytest.raises(ValueError):
        plan_steps([1, 1], 0)


def test_predictor_refuses_a_step_size_below_one_and_imports_without_a_gpu():
    from radargnn_amd.inference import Predictor
    with pytest.raises(ValueError):
        Predictor(object(), [], graphs_per_step=0)
    p = Predictor(object(), [], verbose=False)
    assert p.graphs_per_step == 64 and p.to_host is False and p.verbose is False


# what evaluate.py:6-10 and train.py:6-9 import, name by name
SCRIPT_IMPORTS = [
    ("gnnradarobjectdetection", "postprocessor"),
    ("gnnradarobjectdetection.postprocessor", "evaluation_selector"),
    ("gnnradarobjectdetection.postprocessor.inference", "Predictor"),
    ("gnnradarobjectdetection.postprocessor.postprocessing", "Postprocessor"),
    ("gnnradarobjectdetection.postprocessor.postprocessing", "PredictionExtractor"),
    ("gnnradarobjectdetection.utils.data_handling", "get_data_loaders"),
    ("gnnradarobjectdetection.utils.user_config_reader", "UserConfigurationReader"),
    ("gnnradarobjectdetection.utils.user_config_reader", "ConfigToDataClassMapping"),
    ("gnnradarobjectdetection.utils.user_config_reader", "dataclass_from_dict"),
    ("gnnradarobjectdetection.gnn.gnn_models", "DetNetBasic"),
    ("gnnradarobjectdetection.gnn.trainer", "Trainer"),
    ("gnnradarobjectdetection.gnn.trainer", "set_seeds"),
    ("gnnradarobjectdetection.preprocessor", "config_selector"),
]


@pytest.mark.parametrize("module,name", SCRIPT_IMPORTS)
def test_the_reference_scripts_imports_resolve_under_the_shim(module, name):
    mod = __import__(module, fromlist=[name])              # ``from module import name``: a sub-package counts
    assert hasattr(mod, name), f"{module} has no {name}"


def test_shim_names_are_the_package_objects():
    from gnnradarobjectdetection import preprocessor
    from gnnradarobjectdetection.postprocessor.inference import Predictor
    from gnnradarobjectdetection.utils.user_config_reader import UserConfigurationReader
    from radargnn_amd import config_reader, inference
    from radargnn_amd.nuscenes import NuScenesDatasetConfiguration
    from radargnn_amd.preprocessor import RadarScenesDatasetConfiguration
    assert Predictor is inference.Predictor and UserConfigurationReader is config_reader.UserConfigurationReader
    assert preprocessor.config_selector == {"radarscenes": RadarScenesDatasetConfiguration, "nuscenes": NuScenesDatasetConfiguration}
    assert config_reader.config_selector == preprocessor.config_selector


def _read(name):
    from gnnradarobjectdetection.utils.user_config_reader import UserConfigurationReader
    return UserConfigurationReader.read_config_file(os.path.join(GOLDEN, f"configuration_{name}.yml"))


@pytest.mark.parametrize("dataset", ["radarscenes", "nuscenes"])
def test_shipped_configuration_files_become_the_five_objects(dataset):
    from gnnradarobjectdetection.utils.user_config_reader import ConfigToDataClassMapping, UserConfigurationReader
    from radargnn_amd.gnn.configs import GNNArchitectureConfig, TrainingConfig
    from radargnn_amd.graph_constructor.configs import GraphConstructionConfiguration
    from radargnn_amd.nuscenes import NuScenesDatasetConfiguration
    from radargnn_amd.postprocessor import PostProcessingConfiguration
    from radargnn_amd.preprocessor import RadarScenesDatasetConfiguration
    config = _read(dataset)
    assert set(config) == {"CREATE_DATASET", "TRAIN", "EVALUATE"} and config["CREATE_DATASET"]["dataset"] == dataset
    want = {"DATASET_PROCESSING": {"radarscenes": RadarScenesDatasetConfiguration, "nuscenes": NuScenesDatasetConfiguration}[dataset],
            "GRAPH_CONSTRUCTION": GraphConstructionConfiguration, "MODEL_ARCHITECTURE": GNNArchitectureConfig,
            "TRAINING": TrainingConfig, "POSTPROCESSING": PostProcessingConfiguration}
    classes, super_tasks = ConfigToDataClassMapping.get_mapping_dicts(dataset)
    assert classes == want
    assert super_tasks == {"DATASET_PROCESSING": "CREATE_DATASET", "GRAPH_CONSTRUCTION": "CREATE_DATASET",
                           "MODEL_ARCHITECTURE": "TRAIN", "TRAINING": "TRAIN", "POSTPROCESSING": "EVALUATE"}
    objs = {s: UserConfigurationReader.get_config_object(s, config) for s in SUBSETS}
    for s in SUBSETS:
        assert type(objs[s]) is want[s], s
    if dataset == "radarscenes":
        assert objs["TRAINING"].batch_size == 5
        assert objs["POSTPROCESSING"].iou_for_mAP == 0.3
        assert objs["POSTPROCESSING"].use_point_iou is True
    else:
        assert objs["DATASET_PROCESSING"].nsweeps == 6
        assert objs["TRAINING"].batch_size == 32
    # dict- and list-valued fields arrive as they stand in the file
    assert objs["GRAPH_CONSTRUCTION"].graph_construction_settings == {"k": 20, "r": 1} and objs["GRAPH_CONSTRUCTION"].k == 20
    assert objs["MODEL_ARCHITECTURE"].conv_layer_dimensions == [224, 224, 128, 64, 32]
    assert isinstance(objs["POSTPROCESSING"].min_object_score, dict) and objs["POSTPROCESSING"].min_object_score["car"] > 0


@pytest.mark.parametrize("dataset", ["radarscenes", "nuscenes"])
@pytest.mark.parametrize("subset", SUBSETS)
def test_an_unknown_key_fails_the_conversion(dataset, subset):
    from gnnradarobjectdetection.utils.user_config_reader import ConfigToDataClassMapping, UserConfigurationReader
    config = copy.deepcopy(_read(dataset))
    super_task = ConfigToDataClassMapping.get_mapping_dicts(dataset)[1][subset]
    config[super_task][subset]["no_such_setting"] = 1
    with pytest.raises(Exception, match="Conversion of config file to dataclass failed."):
        UserConfigurationReader.get_config_object(subset, config)


def test_dataclass_from_dict_returns_what_it_cannot_convert():
    from radargnn_amd.config_reader import dataclass_from_dict
    from radargnn_amd.postprocessor import PostProcessingConfiguration
    assert dataclass_from_dict(dict, {"a": 1}) == {"a": 1}
    assert dataclass_from_dict(PostProcessingConfiguration, {"nope": 1}) == {"nope": 1}
    got = dataclass_from_dict(PostProcessingConfiguration, {"split": "test", "bg_index": 0})
    assert isinstance(got, PostProcessingConfiguration) and got.bg_index == 0 and got.iou_for_nms == 0.3


def test_predict_rows_export_checks_its_arguments_before_any_launch():
    """rgnn_predict_rows: no rows is success whatever the pointers; a class count below one, a negative width or leading dimension
    and missing required pointers are refused -- each returns before a launch (the addresses are never dereferenced)."""
    import ctypes as C
    from radargnn_amd import _lib
    f = _lib.lib.rgnn_predict_rows
    d = C.addressof((C.c_double * 64)())
    ok = dict(cls=d, ldc=6, k=6, bb=d, ldb=5, w=5, y=d, ldy=6, f64=1, wy=5, n=4, prob=d, ldp=6, out=d, ldo=5, ct=d, bt=d, ldt=5)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["cls"], a["ldc"], a["k"], a["bb"], a["ldb"], a["w"], a["y"], a["ldy"], a["f64"], a["wy"], a["n"], a["prob"],
                 a["ldp"], a["out"], a["ldo"], a["ct"], a["bt"], a["ldt"], None)

    assert call(n=0) == 0
    assert call(n=0, cls=None, bb=None, y=None, prob=None, out=None, ct=None, bt=None) == 0
    for bad in (dict(k=0), dict(w=-1), dict(wy=-1), dict(n=-1), dict(ldc=-1), dict(ldb=-1), dict(ldy=-1), dict(ldp=-1), dict(ldo=-1),
                dict(ldt=-1), dict(cls=None), dict(prob=None), dict(bb=None), dict(out=None), dict(ct=None), dict(bt=None)):
        assert call(**bad) == -1, bad
        assert b"rgnn_predict_rows" in _lib.lib.rgnn_last_error()
