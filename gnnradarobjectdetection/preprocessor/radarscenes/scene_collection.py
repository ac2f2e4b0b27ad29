from radargnn_amd.preprocessor import SequenceTable, accumulate_frames, plan_windows, scenes_from_rows, subset_windows  # noqa: F401
