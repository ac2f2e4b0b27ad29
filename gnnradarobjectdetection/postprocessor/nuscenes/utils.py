from radargnn_amd.nuscenes_eval import (get_bounding_box_attribute_name, get_bounding_box_detection_name, get_sample_token,  # noqa: F401
                                        get_submission)
