"""orb_slam2_test_amd: MI355X-native (gfx950) ORB-SLAM2 per-frame hot path.

ORBextractor (pyramid, FAST-9 + quadtree distribution, IC_Angle, rBRIEF), ORBmatcher's
Hamming matching (DescriptorDistance, brute-force 2-NN, SearchForInitialization),
Frame::ComputeStereoMatches, the tracking matchers (SearchByProjection), PoseOptimization,
DBoW2's vocabulary transform (Frame::ComputeBoW) and score, KeyFrameDatabase's place
recognition (DetectRelocalizationCandidates, DetectLoopCandidates), Sim3Solver's RANSAC and
Optimizer::OptimizeSim3 (LoopClosing::ComputeSim3), Optimizer::OptimizeEssentialGraph
(LoopClosing::CorrectLoop), Optimizer::GlobalBundleAdjustemnt (a block-sparse Schur solve),
Initializer's H / F RANSAC and two-view reconstruction (Tracking::MonocularInitialization),
the covisibility Map (KeyFrame::UpdateConnections, Tracking::UpdateLocalMap,
MapPoint::UpdateNormalAndDepth),
the LBA Schur solve and
the per-edge arithmetic of Optimizer::LocalBundleAdjustment, as hand-written HIP
kernels behind the C ABI in include/orbg.h (lib/liborbg.so).  The Python classes mirror
the reference's C++ interfaces; see DESIGN.md.
"""
from ._lib import KP_DTYPE, EDGE_DTYPE, EDGE_OUT_DTYPE, POSE_DTYPE, LIB_PATH  # noqa: F401
from .orbextractor import ORBextractor  # noqa: F401
from .orbmatcher import Frame, MapPointProjections, ORBmatcher  # noqa: F401
from .frame import StereoFrame  # noqa: F401
from .optimizer import PoseOptimization, linearize_local_ba, OptimizeSim3, OptimizeSim3Batch  # noqa: F401
from .optimizer import OptimizeEssentialGraph, CorrectMapPoints, EssentialGraph  # noqa: F401
from .optimizer import GlobalBundleAdjustment, CorrectPointsGBA, sparse_symbolic  # noqa: F401
from .vocabulary import ORBVocabulary, BowVector, FeatureVector  # noqa: F401
from .keyframedatabase import KeyFrameDatabase  # noqa: F401
from .sim3solver import Sim3Solver  # noqa: F401
from .pnpsolver import PnPsolver  # noqa: F401
from .initializer import Initializer  # noqa: F401
from .map import Map, MAX_LOOP_EDGES, MAX_LOOP_SET  # noqa: F401

__all__ = ["ORBextractor", "ORBmatcher", "Frame", "MapPointProjections", "StereoFrame", "PoseOptimization", "linearize_local_ba", "OptimizeSim3", "OptimizeSim3Batch",
           "OptimizeEssentialGraph", "CorrectMapPoints", "EssentialGraph",
           "GlobalBundleAdjustment", "CorrectPointsGBA", "sparse_symbolic",
           "ORBVocabulary", "BowVector", "FeatureVector", "KeyFrameDatabase", "Sim3Solver", "PnPsolver", "Initializer", "Map",
           "MAX_LOOP_EDGES", "MAX_LOOP_SET",
           "KP_DTYPE",
           "EDGE_DTYPE", "EDGE_OUT_DTYPE", "POSE_DTYPE"]
