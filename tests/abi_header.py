"""What the host tests of the C ABI share: the header's text, the names a plain regular expression finds declared in it (independent
of the parser in seq2seq_vc_amd/_abi.py), and the built library."""
import os
import re

from seq2seq_vc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text():
    with open(os.path.join(ROOT, "include", "s2svc_hip.h")) as f:
        return f.read()


def declared():
    """Every s2svc_ name followed by `(` anywhere in the header, comments included, minus the struct type names."""
    header = text()
    return set(re.findall(r"\b(s2svc_[a-z0-9_]+)\s*\(", header)) - set(re.findall(r"\}\s*(s2svc_[a-z0-9_]+)\s*;", header))


def library():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library(verbose=False)
    return _lib.lib()
