"""`cramjam.experimental`: where the reference keeps its `blosc2` module (src/experimental.rs) — here the chunk API of cramjam_amd.blosc2."""
import sys as _sys

from cramjam_amd import blosc2  # noqa: F401

_sys.modules[__name__ + ".blosc2"] = blosc2
