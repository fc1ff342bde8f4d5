"""The loader that the ctypes mirrors of the add-on libraries share (large, large_real, large_fir, pfb, pfb_real, large_pfb, pfb_spec, fir_real, fir_detect, bluestein, czt, rowconv, rowconv_real, dct, hilbert, mdct, stft, welch, bands; the polyphase filter banks share more: _pfb_bank.py, the FIR filter banks: _fir_bank.py, the half-length real-row libraries dct, hilbert, mdct, stft, welch and bands: _rows.py): each library is loaded on first
use, so that `import smfft_amd` behaves the same whether it was built or not, and a missing one raises on the first call."""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))


def loader(file_name, env_name, module, sigs):
    """(LIB_PATH, load, lib) of the mirror `module` (its __name__) of smfft_amd/<file_name>; the environment variable env_name names
    another build of it.  load(path) gives a handle typed with sigs = {name: (restype, argtypes)}; lib() loads the module's LIB_PATH
    once and keeps the handle in the module's _lib."""
    def load(path):
        handle = ctypes.CDLL(path)
        for name, (res, args) in sigs.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        return handle

    def lib():
        mod = sys.modules[module]
        if mod._lib is None:
            if not os.path.exists(mod.LIB_PATH):
                raise ImportError(f"{mod.LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                  f"(or `make -C smfft_amd/csrc`).  {module} has no CPU fallback.")
            mod._lib = load(mod.LIB_PATH)
        return mod._lib

    load.__doc__ = f"a typed handle of the {file_name} at `path` (the A/B tools load a second build beside the shipped one)"
    lib.__doc__ = f"the loaded {file_name} (loaded and typed on the first call)"
    return os.environ.get(env_name) or os.path.join(_HERE, file_name), load, lib
