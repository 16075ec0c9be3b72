"""cn_layernorm_c_fwd_f32 / cn_layernorm_c_bwd_f32 for C <= 128 at the edges of the backward kernel's tiling, against the
float64 reference and the bounds of tests/test_norm_gpu.py (_ln_case). The backward walks tiles of 64 pixels; up to 512
tiles every block has one, beyond that a block takes ceil(tiles / 512) (ln_bwd_blocks of cn_norm.hip), and its
parameter gradients are reduced once per block. The chains behind dw / db are no longer here than test_norm_gpu's
ln_param_depth counts: 2 tiles + 6 + 4 + 24 = 36 for 588 and for 513 tiles, against 1 + 6 + 5 + 24."""
import pytest

from test_norm_gpu import _ln_case

pytestmark = pytest.mark.gpu

# shape, residual, output slice, accumulate
TILE_CASES = {
    "35_pixels_C128": ((1, 128, 5, 7), True, False, False),            # fewer than 64 pixels in all
    "198_pixels_C65": ((2, 65, 9, 11), False, True, True),             # 4 tiles, 6 pixels in the last
    "8_tiles_C65": ((2, 65, 16, 16), False, False, False),             # whole tiles, one per block
    "512_tiles_C128": ((4, 128, 64, 128), False, False, True),         # the last size with one tile per block
    "513_tiles_C33": ((3, 33, 96, 114), False, True, False),           # 512 blocks, one of them with two tiles
    "588_tiles_C33": ((3, 33, 111, 113), True, True, True),            # 76 blocks with two tiles, 61 pixels in the last
}


def test_the_tile_counts_are_what_the_names_say():
    for name, (shape, _, _, _) in TILE_CASES.items():
        pixels = shape[0] * shape[2] * shape[3]
        if "tiles" in name:
            assert -(-pixels // 64) == int(name.split("_")[0]), name
        else:
            assert pixels == int(name.split("_")[0]), name
    assert 3 * 111 * 113 % 64 == 61 and 2 * 9 * 11 % 64 == 6 and 3 * 96 * 114 == 513 * 64


@pytest.mark.parametrize("case", list(TILE_CASES), ids=list(TILE_CASES))
def test_layer_norm_f32_tile_edges(case):
    shape, res, out_slice, acc = TILE_CASES[case]
    _ln_case(shape, res=res, out_slice=out_slice, accumulate=acc, edges=True, seed=1200 + len(case), tag=f"ln tiles {case}")
