"""fastselect_amd -- MI355X-native Relief-family feature scoring.

Drop-in for the Relief path of ``fast_select`` (GavinLynch04/FastSelect):
``ReliefF``, ``SURF`` (``use_star=True``: SURF*), ``MultiSURF``
(``use_star=True``: MultiSURF*; also as ``SURFstar`` / ``MultiSURFstar``, the
scikit-rebate names) and the ``TuRF`` meta-estimator, with the same
scikit-learn surface.  Scoring runs in hand-written HIP kernels for gfx950
(``fastselect_amd/csrc``) behind the C ABI in ``include/fastselect_amd.h``;
``fastselect_amd.parallel`` shards MultiSURF over one process per GPU.
``MDR`` is the reference's exhaustive k-way SNP interaction search, the usual
second stage after a Relief filter (``MDR.rank_interactions``: the ranked list
of the n_top best interactions, not only the winner); ``mRMR`` (with the
``fastselect_amd.mutual_information`` functions it is built on) drops
redundant features in between, ``CFS`` picks a subset by correlation with
the class against correlation within the subset, and ``JMI`` (JMI / CMIM) selects
by joint relevance, which keeps features that matter only in interaction;
``PairScreen`` (``mutual_information.rank_pair_interactions``) scans all pairs
for the ones that act purely together and returns them as a ranked list.
``RReliefF`` scores features against a continuous target (the Relief
estimators above read y as class labels), with a permutation test.

Importing the package loads the native library; it fails loudly if the
library has not been built.
"""
from . import _lib, mutual_information
from .CFS import CFS
from .JMI import JMI
from .MDR import MDR
from .mRMR import mRMR
from .MultiSURF import MultiSURF
from .PairScreen import PairScreen
from .ReliefF import ReliefF
from .RReliefF import RReliefF
from .SURF import SURF
from .star import MultiSURFstar, SURFstar
from .TuRF import TuRF

# The classes shadow their defining submodules here (``fastselect_amd.SURF`` is
# the class, not the module), so a pickler that resolves ``__module__`` by
# attribute access cannot find them there and serialises the class by value:
# dill does, and once a package that uses it (multiprocess, datasets) is
# imported, so does joblib.dump.  Name the estimators by their public address.
for _cls in (MultiSURF, ReliefF, RReliefF, SURF, TuRF, MDR, mRMR, CFS, JMI, PairScreen):
    _cls.__module__ = __name__
del _cls

__version__ = "0.1.0"
__all__ = ["ReliefF", "RReliefF", "SURF", "MultiSURF", "SURFstar", "MultiSURFstar", "TuRF", "MDR", "mRMR",
           "CFS", "JMI", "PairScreen"]


def gpu_available() -> bool:
    """True when at least one HIP device is visible to the native library."""
    return _lib.gpu_available()
