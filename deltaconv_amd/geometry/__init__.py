from .operators import *          # noqa: F401,F403
from .grad_div_mls import *       # noqa: F401,F403
from .graph import Graph, knn_graph, as_graph  # noqa: F401
from .utils import batch_dot      # noqa: F401
from . import fps                                    # noqa: F401  (the module; calling it IS fps.fps: geometry.fps(pos, ...))
from .fps import geodesic_fps, geodesic_fps_batch    # noqa: F401
from .mesh_sample import sample_points_batch         # noqa: F401
from .shape_norm import normalize_shapes_batch       # noqa: F401
from .mesh_normals import vertex_face_lists, vertex_normals_batch    # noqa: F401
from .interpolate import interpolate_rows_backward, knn_cross, knn_cross_transpose, knn_interpolate  # noqa: F401
from .connection import *         # noqa: F401,F403
from .vector_interpolate import *  # noqa: F401,F403
from .pool import *               # noqa: F401,F403
from .pool_vectors import *       # noqa: F401,F403
from .resample import CloudPair, fps_levels, prefix_levels    # noqa: F401
from .voxel import voxel_subsample                   # noqa: F401
from .cluster import *            # noqa: F401,F403
from .cluster_vectors import *    # noqa: F401,F403
