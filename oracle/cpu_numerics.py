"""One CPU numeric path for everything that is pinned bit for bit against `tests/golden/`.

The CPU oracle (oracle/refpath.py) must reproduce vectors captured from the imported reference bit for bit.  Its
products run in MKL and its elementwise / reduction kernels in ATen, and both pick their code path at run time: MKL
by CPU vendor and ISA (an Intel AVX-512 host and an AMD one differ in the last bits), MKL's conditional-reproducibility
path additionally by thread count, ATen by ISA.  Fixing all three before torch is loaded gives the same bits on any
x86-64 host with AVX2.  `tests/conftest.py`, `make_golden_submodules.py` and `make_golden.py --cpu-pinned` (which writes
tests/golden/cpu_pinned/) call `pin()` before torch is imported.
"""
import os

SETTINGS = {
    "MKL_CBWR": "COMPATIBLE",       # MKL's vendor- and ISA-independent code path
    "ATEN_CPU_CAPABILITY": "avx2",  # ATen's vector kernels at AVX2 width on every host
    "OMP_NUM_THREADS": "8",         # the compatible path splits products by thread count
}


def pin():
    """Set the environment of the pinned path.  Takes effect only if torch has not been imported yet."""
    os.environ.update(SETTINGS)


def is_pinned():
    """True if the torch of this process runs on the pinned path (it was imported after `pin()`)."""
    import torch
    return (os.environ.get("MKL_CBWR") == SETTINGS["MKL_CBWR"]
            and torch.backends.cpu.get_cpu_capability() == SETTINGS["ATEN_CPU_CAPABILITY"].upper()
            and torch.get_num_threads() == int(SETTINGS["OMP_NUM_THREADS"]))
