"""Drop-in for ``rfi_toolbox.preprocessing`` (reference preprocessing/preprocessor.py)."""
from .normalization import Normalizer, invalid_map, normalize_array
from .preprocessor import Preprocessor, patchify

__all__ = ["Preprocessor", "patchify", "Normalizer", "normalize_array", "invalid_map"]
