"""libdisprcnn_pts.so: the 3D stage's point ops (instance point clouds, PointNet++), a library apart from the regressor's."""
