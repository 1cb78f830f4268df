"""MI355X-native forward/backward for a CTR model zoo."""
__version__ = "0.1.0"

from .cf import ItemCF, UserCF, implicit_matrix, recall_precision_f1  # noqa: E402,F401
from .gdcf import GDCF  # noqa: E402,F401
from .als import ALS  # noqa: E402,F401
