"""Core RFI simulation (the reference's ``rfi_toolbox.core``): ``RFISimulator`` generating its four-polarisation
waterfalls and full-truth masks on the GPU (csrc/rfi_sim.hip), and the per-emitter instance targets of a generated batch
(``event_table``, ``event_instances``)."""
from .instances import EVENT_CLASSES, event_instances, event_table, family_masks
from .simulator import EVENT_DTYPE, RFISimulator, SimBatch, SimOrigin, event_slots

__all__ = ["RFISimulator", "SimBatch", "SimOrigin", "EVENT_DTYPE", "event_slots", "event_table", "event_instances", "family_masks", "EVENT_CLASSES"]
