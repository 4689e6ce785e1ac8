"""Developer tool: bench.py with another build of the library, for before / after runs on one box (bench.py itself always loads
the in-tree library):

    CTPVAE_VARIANT_LIB=tools/libctpvae_radon_<tag>.bin python tools/bench_variant.py --gpus 1 --steps 20 --warmup 20

The variant is an older build of the same C ABI (tools/build_variant.sh); entry points added since are dropped from the binding
table -- bench.py's timed steps call none of them.  Without CTPVAE_VARIANT_LIB this is `python bench.py` through the same door."""
import ctypes
import os
import runpy
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ct_pvae_amd import _lib

if os.environ.get("CTPVAE_VARIANT_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["CTPVAE_VARIANT_LIB"])
    _old = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(_old, k)}
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
