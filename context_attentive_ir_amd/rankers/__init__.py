from .esm import ESM
from .mtensor import MatchTensor
from .drmm import DRMM
from .duet import DUET
from .dssm import DSSM
from .cdssm import CDSSM
from .arci import ARCI
from .arcii import ARCII

__all__ = ["ESM", "MatchTensor", "DRMM", "DUET", "DSSM", "CDSSM", "ARCI", "ARCII"]
