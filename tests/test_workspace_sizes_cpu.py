"""The size queries of the library against recorded values: every layout carves its workspace with the one cursor of
g4s_internal.h (WorkspaceCursor), and a change to it, or to one layout's own + 256 convention, must not move an offset or
a size that callers and saved states already depend on.  Host-side only: no query touches the device."""
import ctypes

import pytest

from g4splat_amd._lib import G4sLayout

# Recorded from the library of commit 5841477 ("Test the marching-cubes kernels on noise, holes, gaps and key edges"),
# the last one in which every layout function had its own `take` lambda.
SIZES = {
    "g4s_tsdf_workspace": [((64, 48, 7, 0), 869120), ((1600, 1200, 10, 0), 772878080), ((0, 0, 0, 1), 3840),
                           ((0, 0, 0, 1025), 2117376)],
    "g4s_dense_mc_workspace": [((1,), 0), ((2,), 2304), ((33,), 76032), ((257,), 35012608), ((1024,), 2214609664)],
    "g4s_utsdf_workspace": [((0,), 256), ((5,), 696)],
    "g4s_atsdf_workspace": [((0,), 256), ((5,), 1016)],  # newer than that commit: 5 records of 152 bytes + 256
    "g4s_mesh_cluster_workspace": [((0,), 256), ((1,), 13056), ((171,), 26368), ((1000,), 106752), ((334000,), 27838208)],
    "g4s_mesh_compact_workspace": [((0, 0), 768), ((1, 1), 1792), ((500, 1000), 13056)],
    "g4s_knn_workspace": [((0,), 4096), ((1,), 6144), ((257,), 14336), ((100000,), 3308032)],
    # Recorded from the library of commit 03db0f4 ("One core for the chart units"), the last one before the units that
    # sum in a fixed order took their sums from csrc/fixed_sums.h: no partial-row layout moved with them.
    "g4s_photometric_workspace": [((0, 0), 0), ((33, 17), 20736), ((1600, 1200), 69300480)],
    "g4s_geometry_regularizers_workspace": [((0, 0), 256), ((33, 17), 512), ((1600, 1200), 15360)],
    "g4s_chart_prior_workspace": [((0, 0), 0), ((33, 17), 5120), ((1025, 1000), 8283136)],
    "g4s_anisotropy_workspace": [((0,), 0), ((257,), 512), ((1048577,), 16896)],
    "g4s_chart_match_workspace": [((0, 0, 0), 0), ((3, 17, 33), 14080), ((6, 240, 320), 3694080)],
    "g4s_chart_align_workspace": [((0, 0, 0), 0), ((3, 17, 33), 61440), ((2, 1024, 513), 37954048)],
    "g4s_chart_points_workspace": [((0, 0, 0, 0), 0), ((3, 17, 33, 1000), 8704), ((6, 240, 320, 100000), 801792)],
    "g4s_plane_fit_members_workspace": [((0, 0, 0), 1024), ((1000, 3, 5), 9728), ((2000000, 40, 60), 16009472)],
}
# (P, R, width, height) -> every field of G4sLayout, in declaration order
LAYOUTS = [
    ((0, 0, 1, 1), (0, 0, 0, 0, 6912, 256, 2560, 3328, 0, 256, 512, 768, 2304, 1536)),
    ((1, 3, 33, 17), (0, 256, 2048, 512, 11264, 256, 3584, 4352, 0, 256, 7168, 11776, 13312, 12544)),
    ((257, 5000, 1600, 1200),
     (0, 33024, 42240, 33536, 52480, 0, 84480, 94976, 0, 60160, 23100160, 38460160, 38611456, 38580736)),
]


@pytest.mark.parametrize("name", sorted(SIZES))
def test_workspace_sizes_are_the_recorded_ones(hip_lib, name):
    for args, want in SIZES[name]:
        assert getattr(hip_lib, name)(*args) == want, (name, args)


def test_rasterizer_layout_is_the_recorded_one(hip_lib):
    for args, want in LAYOUTS:
        lay = G4sLayout()
        assert hip_lib.g4s_rasterizer_layout(*args, ctypes.byref(lay)) == 0, args
        got = {f: getattr(lay, f) for f, _ in G4sLayout._fields_}
        assert got == dict(zip((f for f, _ in G4sLayout._fields_), want)), args
