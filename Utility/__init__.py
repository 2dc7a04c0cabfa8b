"""The reference's ``Utility`` package path.  This repository provides ``Utility.Scorer`` only; with the reference's checkout also on
``sys.path`` its other modules (``Utility.storage_config``, ``Utility.utils``, ...) stay importable from there."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
