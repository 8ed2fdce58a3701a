"""frame_planes with the refinement on and off (k_f360_moments + k_f360_refine_commit) at W x W/2, 20 calls each: python tools/prof_plane_sums.py ROOT W
(ROOT: the tree whose library is loaded; run under rocprofv3 --kernel-trace --stats)"""
import os, sys
root = os.path.abspath(sys.argv[1]); W = int(sys.argv[2])
sys.path.insert(0, root)
from rgbd360_amd import synth
from rgbd360_amd.register import RegisterPhotoICP, Frame360Stages
import rgbd360_amd._lib as L
print("lib", L.__file__)
dA = synth.make_pair(W, W // 2, seed=5)[0][1]
st = Frame360Stages(RegisterPhotoICP())
for refine in (False, True):
    st.set_refinement(refine, 0.02)
    for _ in range(20):
        out = st.frame_planes(dA, convention=2, angular_threshold=0.03 * 1024 / W, min_inliers=40, max_curvature=0.0013, max_planes=4096)
    print("refine", refine, "planes", len(out["planes"]), st.refinement_stats())
