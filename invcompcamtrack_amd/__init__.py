"""MI355X-native Gauss-Newton photometric camera tracker (drop-in for catree/InvCompCamTrack's
per-frame tracking hot path). See DESIGN.md. The HIP library is loaded lazily by ``_lib.load()``;
importing this package never touches the GPU and never falls back to a CPU implementation."""
from . import _lib  # noqa: F401
from ._lib import IctrError  # noqa: F401
from ._lib import REF8_DIRECT_TAPS  # noqa: F401
from ._lib import (VARIANT_ALL, VARIANT_ANY_SIZE, VARIANT_DEBUG_MUTE, VARIANT_DYNAMIC_LOOP, VARIANT_GRAD_PLANES,  # noqa: F401
                   VARIANT_H_BY_SETUP, VARIANT_LAUNCHES, VARIANT_NO_GRAPH, VARIANT_NO_RESIDENT, VARIANT_NO_TEAMS,
                   VARIANT_ONE_LAUNCH, VARIANT_SEPARATE_BEGIN)
from .tracker import (CamClass, OdometerClass, PoseClass, Pyramid, TrackBatch, device_count, locality_order, ncc_score, optparam,  # noqa: F401
                      timebase_mark,
                      solve6,
                      util_constructpyramide, util_getPatch, util_getPatch_grad, util_SE3_coeff_to_group,
                      util_SE3_group_to_coeff)
from .ransac import fit_cameras_odom, sample_poses, sample_poses_host  # noqa: F401
from .fsplit import (StaticSplitter, epiline_dist, fit_f8, pairs_from_stereo_tracks, pairs_from_tracks, split_static,  # noqa: F401
                     split_static_host)
from .camfit import (CameraFitter, depth_from_disparity, fit_cameras, fit_cameras_host,  # noqa: F401
                     observations_from_stereo_tracks, points_from_first_view, reprojection_errors,
                     reprojection_errors_host)
from .stereotrack import (StereoPointTracker, StereoTrackWindow, stereo_track_window,  # noqa: F401
                          stereo_track_window_host)
from .windowcams import cameras_from_tracks, cameras_from_window, window_cameras, window_cameras_host  # noqa: F401
from .windowcams import bundle_from_window, window_bundle_host  # noqa: F401
from .windowcams import ransac_cameras, ransac_cameras_from_window, window_ransac_cameras_host  # noqa: F401
from .camransac import CameraRansac, window_ransac, window_ransac_host  # noqa: F401
from .bundle import BundleAdjuster, adjust_window, adjust_window_host  # noqa: F401
from .triang import Triangulator, cameras_from_poses, rays_from_first_view, tracks_from_oftrack, triangulate_tracks  # noqa: F401
from .sequence import SequenceTracker, select_points, track_sequence, track_sequence_host_loop  # noqa: F401

__version__ = "0.1.0"
