"""lidar_slam_amd — MI355X-native per-scan hot path of Farofeiro231/LiDAR_SLAM.

RANSAC line/landmark extraction (ransac_functions.py / landmarking.py, with
scikit-image 0.18.3 ``ransac``/``LineModelND`` semantics and numpy's legacy
MT19937 stream) and the intended UKF predict/update (UKFMethods.py /
systemClass.py with filterpy semantics), as hand-written HIP kernels for
gfx950 behind a C ABI (include/lidarslam.h) loaded with ctypes.

Drop-in modules mirror the reference's call surface:
  lidar_slam_amd.ransac_functions  landmark_extraction / check_ransac
  lidar_slam_amd.landmarking       Landmark
  lidar_slam_amd.systemClass       System (.ukf.predict / .ukf.update)
  lidar_slam_amd.functions         polar->Cartesian + chunking of a revolution
Batched API: lidar_slam_amd.pipeline.ScanPipeline, lidar_slam_amd.slam.LandmarkMap,
lidar_slam_amd.odometry.ScanMatcher / LidarOdometry (LiDAR-only odometry: wheel speeds from the scans),
lidar_slam_amd.mapping.OccupancyGrid (per-robot log-odds grids from the revolutions and the filter's poses;
``recentre`` rolls a grid under a robot that nears its edge; ``merge`` folds another robot's map into it under
``mapping.merge_transform``, gated on the two maps' agreement),
lidar_slam_amd.mapping.GridScan (a map as a revolution: a grid's occupied cells about an anchor pose, on the device,
in the form every matcher takes) and lidar_slam_amd.mapping.align_maps (that scan relocalised in another map: the
merge's transform found from the two maps alone),
lidar_slam_amd.mapping.GridRayCaster (the grid read beam by beam: expected returns, beam classes, the dynamic-object mask),
lidar_slam_amd.mapping.DistanceField (the grid's exact distance field: clearance, a revolution's distance to the map,
its Gauss-Newton alignment there, and ``fuse``: that alignment as a gated Kalman update of the filter),
lidar_slam_amd.localize.GridLocalizer (scan-to-map matching: the pose corrected against the robot's grid),
lidar_slam_amd.localize.GridRelocalizer (global relocalisation: the pose found in the grid without a guess),
lidar_slam_amd.posegraph.PoseGraph (loop closure: a pose graph per robot optimised on the device, with
``posegraph.relative_pose`` and ``posegraph.closure_edge`` for its edges; ``OccupancyGrid.redraw`` draws the map again
from the corrected keyframes; ``PoseGraph.propose`` and ``PoseGraph.gate`` judge closure candidates by their innovation
against the graph before they become edges, ``PoseGraph.relative_covariance`` with ``posegraph.closure_window`` gives the
window in which to look for a closure).
"""
__version__ = "0.1.0"
