from radargnn_amd.nuscenes import extended_points_in_box  # noqa: F401
