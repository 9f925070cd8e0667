"""One CPU arithmetic for the test suite and for the fixture generators under tests/golden/.

torch picks its CPU kernels by the host's instruction set (ATen's SIMD level) and MKL picks a code path per processor, so the
same float32 computation, random draws included, can differ in the last bits between two x86-64 hosts (an Intel AVX-512 host
and an AMD host do). Fixtures that pin CPU-computed values bit for bit are therefore captured, and checked, under one setting
that every x86-64 host with AVX2 runs alike: ATen's AVX2 kernels and MKL's COMPATIBLE branch. Both are read when torch runs
its first kernel: apply() before torch is imported (tests/conftest.py, tests/golden/make_*_fixture*.py). The generators also
run on one thread: some GEMMs that produce stored inputs split their sums differently over other thread counts."""
import os

SETTINGS = {"ATEN_CPU_CAPABILITY": "avx2", "MKL_CBWR": "COMPATIBLE"}


def apply(threads=None) -> None:
    os.environ.update(SETTINGS)
    if threads is not None:
        os.environ["OMP_NUM_THREADS"] = str(threads)
