from radargnn_amd.gnn.trainer import Trainer, get_new_result_folder_path, set_seeds  # noqa: F401
