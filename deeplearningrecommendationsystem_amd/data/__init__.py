from .features import FeatureAssembler
from .leave_one_out import LeaveOneOut
from .loader import DeviceLoader, ObservedPairs

__all__ = ["FeatureAssembler", "DeviceLoader", "LeaveOneOut", "ObservedPairs"]
