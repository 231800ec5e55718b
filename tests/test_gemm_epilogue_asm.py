"""The store epilogue of the bf16-split GEMM kernels on the final ISA (tools/check_gemm_epilogue_asm.py): no vector-memory load and no
wait that names vmcnt inside the store passes of any k_gemm_bx3 / k_gemm_bx3w / k_gemm_bx3h instantiation, no scratch, and two waves per
SIMD for the 256-tile kernel.  hipcc cross-compiles without a GPU."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc is not installed')
def test_store_passes_hold_no_load_and_no_vmcnt_wait():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_gemm_epilogue_asm.py')], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True, timeout=900)
    print(proc.stdout[-6000:])
    assert proc.returncode == 0, proc.stdout[-3000:]
