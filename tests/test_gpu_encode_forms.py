"""The streaming encoder's knob-only forms on the MI355X (encode_forms_common.py): LERC_AMD_ENCODE_LAUNCHES=2 -- one raster in two
launches at a size that takes more than one scan slice and pack group, a ragged raster, a band stack, a tile batch in three launches,
slotted, and with an arena one byte too small -- and LERC_AMD_TILE_ARENA=copy, the one-launch tile batch with a slot a tile, which
the GPU's default (tiles claim their room in the arena themselves) never runs."""
import pytest

import encode_forms_common as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("check", ["single_rasters", "ragged_raster", "band_stack", "tile_batch"])
def test_two_launch_forms(check):
    C.run("gpu", [check], LERC_AMD_ENCODE_LAUNCHES="2")


def test_tile_batch_that_copies_its_slots():
    C.run("gpu", ["copy_arena"], LERC_AMD_TILE_ARENA="copy")
