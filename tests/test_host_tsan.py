"""ThreadSanitizer run of the library's threaded HOST code (no GPU): tests/tsan_driver.cpp + ballermixplus_amd/csrc/bmx_io.cpp
compiled with g++ -fsanitize=thread -- the input reader (one byte range per thread), the validation passes of
bmx_ctx_set_sites / bmx_ctx_set_tests (std::atomic fault flags), and the multi-threaded row formatter of bmx_write_rows /
bmx_write_records.  GPU AddressSanitizer / XNACK runs are not available on the GPU pool; sanitizers run on the CPU build."""
import os
import platform
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_host_threads_are_race_free_under_tsan(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'tsan_driver')
    r = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=thread', '-pthread', '-o', exe,
                        os.path.join(HERE, 'tsan_driver.cpp'), os.path.join(REPO, 'ballermixplus_amd', 'csrc', 'bmx_io.cpp')],
                       capture_output=True, text=True)
    if r.returncode != 0 and 'tsan' in r.stderr.lower() and 'cannot find' in r.stderr.lower():
        pytest.skip('libtsan is not installed')
    assert r.returncode == 0, r.stderr[-3000:]
    cmd = [exe, str(tmp_path)]
    # GCC's ThreadSanitizer runtime knows the address layout of a process only for the usual mmap randomisation; on kernels that
    # randomise with more bits (vm.mmap_rnd_bits = 32) it stops at start-up with "unexpected memory mapping".  Where races are
    # found does not depend on where the process is mapped, so the driver runs with address randomisation off for itself.
    setarch = shutil.which('setarch')
    if setarch and subprocess.run([setarch, platform.machine(), '-R', 'true'], capture_output=True).returncode == 0:
        cmd = [setarch, platform.machine(), '-R'] + cmd
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, TSAN_OPTIONS='halt_on_error=0 report_signal_unsafe=0'))
    assert 'ThreadSanitizer' not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and 'tsan driver ok' in run.stdout, (run.stdout[-500:], run.stderr[-2000:])
