#!/usr/bin/env python3
"""Drop-in command for `python BalLeRMix+_v1.py ...` (same flags) running the scan on MI355X."""
import os
import sys
import threading


def _prewarm():
    """First HIP call of the process (runtime start-up, ~0.25 s) on a helper thread, before the Python imports and the argument
    parsing: the context the scan creates later finds the runtime up."""
    try:
        import ctypes
        here = os.path.dirname(os.path.abspath(__file__))
        ctypes.CDLL(os.path.join(here, 'ballermixplus_amd', os.environ.get('BMX_LIB_NAME', 'libbmxscan.so'))).bmx_device_count()
    except Exception:           # a missing or stale library is reported by the scan itself
        pass


_warm = None
if __name__ == '__main__' and len(sys.argv) > 1 and not any(a in sys.argv for a in ('--getSpect', '--getConfig', '-h', '--help')):
    _warm = threading.Thread(target=_prewarm, daemon=True)
    _warm.start()

from ballermixplus_amd.cli import main  # noqa: E402

if __name__ == '__main__':
    try:
        main()
    except BaseException:
        # An early way out (a refusal of the arguments and its sys.exit(1), an uncaught exception) can end the run within
        # milliseconds, while the helper thread is still inside the HIP runtime's start-up; the interpreter then tore the process
        # down under it (once seen as a SIGSEGV after the refusal was printed).  Wait for the thread, then leave as before.
        if _warm is not None:
            _warm.join()
        raise
    # Every output file is written, closed and (multi-process runs) the process group destroyed by now.  Tearing down the HIP
    # runtime and Python takes ~0.1 s of a 0.75 s run on a 1M-SNP file; BMX_FAST_EXIT=0 keeps the orderly shutdown.
    sys.stdout.flush()
    sys.stderr.flush()
    if os.environ.get('BMX_FAST_EXIT', '1') != '0':
        os._exit(0)
