"""Drop-in for ``rfi_toolbox.preprocessing`` (reference preprocessing/preprocessor.py)."""
from .normalization import Normalizer, normalize_array
from .preprocessor import Preprocessor, patchify

__all__ = ["Preprocessor", "patchify", "Normalizer", "normalize_array"]
