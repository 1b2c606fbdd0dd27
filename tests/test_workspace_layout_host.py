"""Every workspace query of the scene-side modules against literal byte counts (no GPU: the library loads without one).

The layouts are part of the C ABI: callers size their buffers with these functions, and Python reads the stereo volume at
mvsdf_stereo_volume_offset.  The numbers in EXPECTED were taken from a library built from the parent of the commit that moved the layout
functions onto csrc/geom_prims.h (WsCursor, mv_align256, mv_scan_tmp_bytes), by running this file as a script against it:

    MVSDF_LIB=<that library> python tests/test_workspace_layout_host.py

which prints the dict below.  Shapes per function: the smallest accepted one, sizes just below, at and above a multiple of the 2048-item scan
chunk (1024 for the marching-cubes passes), one large shape, and the refused shapes (0) the other host tests list.  mvsdf_trace_workspace_bytes_n was added
the same way from the parent of the commit that moved the tracer's layout into csrc/trace_route.h (MvTraceWs)."""
import pytest

I31 = 2 ** 31 - 1

SHAPES = {
    'mvsdf_mc_workspace_bytes': [(2, 2, 2), (17, 31, 9), (2, 3, 341), (2, 2, 512), (2, 5, 205), (512, 512, 512),
                                 (1, 5, 5), (5, 0, 5), (5, 5, -3), (1 << 21, 1 << 21, 1 << 21), (1 << 40, 1 << 40, 2)],
    'mvsdf_mesh_cc_workspace_bytes': [(1, 1), (100, 196), (2047, 2049), (2048, 2048), (2049, 2047), (I31, I31),
                                      (0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31)],
    'mvsdf_smc_workspace_bytes': [(3, 2), (100, 8), (2048, 8), (2048, 16), (129, 2), (257, 2), (2580, 2),
                                  (2, 8), (3, 1), (100, 0), (100, -4), (100, 2000), (1 << 40, 8), (3000, 2)],
    'mvsdf_smc_emit_workspace_bytes': [(3, 2, 1), (100, 8, 5), (100, 3, 127), (100, 3, 128), (100, 3, 129), (100, 8, 13 ** 3), (2048, 8, 1000000),
                                       (100, 8, 0), (100, 8, 13 ** 3 + 1), (2, 8, 1)],
    'mvsdf_mesh_cut_workspace_bytes': [(1, 1), (100, 196), (2047, 2049), (2048, 2048), (2049, 2047), (I31, I31 // 8),
                                       (0, 5), (5, 0), (1 << 31, 5), (5, I31 // 8 + 1)],
    'mvsdf_chamfer_sample_workspace_bytes': [(1, 1), (8, 2047), (8, 2048), (8, 2049), (I31, I31), (0, 1), (1, 0), (1 << 31, 1), (1, 1 << 31)],
    'mvsdf_chamfer_downsample_workspace_bytes': [(1,), (1023,), (1024,), (1025,), (2047,), (2048,), (2049,), (I31 // 4,), (0,), (-1,), (I31 // 4 + 1,)],
    'mvsdf_chamfer_mask_workspace_bytes': [(1, 1), (2047, 2049), (2048, 2048), (2049, 2047), (1 << 40, 1 << 40),
                                           (0, 1), (1, 0), ((1 << 40) + 1, 1), (1, (1 << 40) + 1)],
    'mvsdf_chamfer_nearest_workspace_bytes': [(0, 1), (1, 1), (2047, 2049), (2048, 2048), (2049, 2047), (4095, 4097), (1 << 40, I31),
                                              (-1, 1), (1, 0), ((1 << 40) + 1, 1), (1, 1 << 31)],
    'mvsdf_fusion_workspace_bytes': [(1, 2, 2, 0), (1, 23, 89, 2), (1, 2, 1024, 1), (1, 3, 683, 2), (2, 32, 33, 4), (49, 1200, 1600, 490),
                                     (1, 1, 4, 2), (0, 4, 4, 0), (1, 4, 1, 0), (1, 4, 4, -1), (1, 65536, 32768, 0), (1 << 31, 4, 4, 0),
                                     (1024, 32768, 32768, 0)],
    'mvsdf_cloud_clean_workspace_bytes': [(2,), (2047,), (2048,), (2049,), (4097,), (I31,), (1,), (0,), (1 << 31,)],
    'mvsdf_cloud_compact_workspace_bytes': [(1,), (2047,), (2048,), (2049,), (2048 * 1024 + 2049,), (I31,), (0,), (-1,), (1 << 31,)],
    'mvsdf_raster_workspace_bytes': [(0, 0, 1, 2, 2), (1, 1, 1, 2, 2), (10, 2047, 1, 4, 4), (10, 512, 4, 4, 4), (10, 683, 3, 4, 4),
                                     (100000, 200000, 49, 1200, 1600),
                                     (-1, 1, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 65536, 4, 4), (1, 1, 1, 1, 4), (1, 1, 1, 4, 1), (2 ** 31, 1, 1, 4, 4),
                                     (1, 2 ** 30, 2, 4, 4), (1, 1, 1, 2 ** 16, 2 ** 15)],
    'mvsdf_stereo_workspace_bytes': [(2, 2, 1, 0), (16, 16, 4, 2), (23, 89, 1, 3), (32, 64, 1, 3), (3, 683, 1, 3), (1200, 1600, 192, 10),
                                     (1, 16, 4, 2), (16, 16, 0, 2), (16, 1, 4, 2), (16, 16, 65536, 2), (16, 16, 4, -1), (65536, 32768, 1, 0),
                                     (32768, 32768, 1025, 0)],
    'mvsdf_viewsel_workspace_bytes': [(1,), (2,), (64,), (65,), (65535,), (0,), (-1,), (65536,)],
    'mvsdf_trace_workspace_bytes_n': [(1, 2), (17, 100), (2048, 128), (8193, 1024), (0, 100), (-5, 100), (17, 0)],
}
SHAPES['mvsdf_stereo_volume_offset'] = SHAPES['mvsdf_stereo_workspace_bytes']

EXPECTED = {
    'mvsdf_chamfer_downsample_workspace_bytes': [2816, 76544, 76544, 143104, 152320, 152320, 284416, 39732642560, 0, 0, 0],
    'mvsdf_chamfer_mask_workspace_bytes': [2048, 50688, 50432, 50944, 26401163969792, 0, 0, 0, 0],
    'mvsdf_chamfer_nearest_workspace_bytes': [3840, 3840, 109312, 107776, 107776, 214528, 119149425408, 0, 0, 0, 0],
    'mvsdf_chamfer_sample_workspace_bytes': [1024, 17152, 17152, 17408, 17188258560, 0, 0, 0, 0],
    'mvsdf_cloud_clean_workspace_bytes': [4608, 140288, 140288, 142848, 280832, 144919229440, 0, 0, 0],
    'mvsdf_cloud_compact_workspace_bytes': [1024, 17152, 17152, 17408, 16802816, 17188258560, 0, 0, 0],
    'mvsdf_fusion_workspace_bytes': [2048, 20224, 19968, 20736, 21504, 847222016, 0, 0, 0, 0, 0, 0, 0],
    'mvsdf_mc_workspace_bytes': [1536, 20480, 9472, 9472, 9728, 540016896, 0, 0, 0, 0, 0],
    'mvsdf_mesh_cc_workspace_bytes': [3328, 5376, 59136, 59136, 60672, 60179874560, 0, 0, 0, 0],
    'mvsdf_mesh_cut_workspace_bytes': [6400, 41216, 356352, 354560, 356352, 106328753408, 0, 0, 0, 0],
    'mvsdf_raster_workspace_bytes': [1280, 1280, 11008, 11264, 11776, 801678848, 0, 0, 0, 0, 0, 0, 0, 0],
    'mvsdf_smc_emit_workspace_bytes': [1280, 15616, 33536, 33792, 34048, 6411264, 2917898496, 0, 0, 0],
    'mvsdf_smc_workspace_bytes': [1792, 62976, 469958912, 58745088, 7343360, 58745088, 60132449280, 0, 0, 0, 0, 0, 0, 0],
    'mvsdf_stereo_volume_offset': [768, 768, 1024, 1024, 1024, 1792, 0, 0, 0, 0, 0, 0, 0],
    'mvsdf_stereo_workspace_bytes': [1280, 9984, 19456, 19456, 19968, 3317761792, 0, 0, 0, 0, 0, 0, 0],
    'mvsdf_viewsel_workspace_bytes': [264, 288, 33024, 34056, 34358690056, 0, 0, 0],
    'mvsdf_trace_workspace_bytes_n': [316, 14604, 2187520, 67477804, 256, 256, 1004],
}
EMPTY = {'mvsdf_trace_workspace_bytes_n': 256}       # this query refuses nothing: no rays = its 256 bytes of slack (every other one answers 0 to a refused shape)


def _table():
    from mvsdf_amd import _lib
    L = _lib.lib()
    return {fn: [int(getattr(L, fn)(*shape)) for shape in shapes] for fn, shapes in sorted(SHAPES.items())}


@pytest.mark.parametrize('fn', sorted(SHAPES))
def test_workspace_bytes_are_the_recorded_ones(fn):
    from mvsdf_amd import _lib
    f = getattr(_lib.lib(), fn)
    assert len(EXPECTED[fn]) == len(SHAPES[fn]) >= 6
    assert any(x == EMPTY.get(fn, 0) for x in EXPECTED[fn]) and sum(1 for x in EXPECTED[fn] if x != EMPTY.get(fn, 0)) >= 5      # refusals and accepted shapes are both pinned
    for shape, want in zip(SHAPES[fn], EXPECTED[fn]):
        assert int(f(*shape)) == want, (fn, shape)


if __name__ == '__main__':
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    print('EXPECTED = {')
    for fn, row in _table().items():
        print('    %r: %r,' % (fn, row))
    print('}')
