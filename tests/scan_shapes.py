"""The sizes of vdjer_amd/csrc/vdjx_scan.h, read from the header itself: the one-launch tile per output width and the device-wide
block.  The edge cases of tests/test_gpu_scan.py and tests/test_gpu_quant.py are placed around them."""
import os
import re

_H = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vdjer_amd", "csrc", "vdjx_scan.h")).read()


def _define(name):
    (v,) = re.findall(r"^#define %s (\d+)u\b" % name, _H, re.M)
    return int(v)


TILE = {False: _define("VDJX_SCAN_TILE_U32"), True: _define("VDJX_SCAN_TILE_U64")}      # by "the output is u64"
BLOCK = _define("VDJX_SCAN_BLOCK")
