"""Core RFI simulation (the reference's ``rfi_toolbox.core``): ``RFISimulator`` generating its four-polarisation
waterfalls and full-truth masks on the GPU (csrc/rfi_sim.hip)."""
from .simulator import EVENT_DTYPE, RFISimulator, SimBatch, event_slots

__all__ = ["RFISimulator", "SimBatch", "EVENT_DTYPE", "event_slots"]
