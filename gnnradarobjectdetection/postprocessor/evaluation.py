from radargnn_amd.metrics import Evaluator, get_new_evaluation_folder_path  # noqa: F401
