"""The CPU segment engine (TEST INFRASTRUCTURE, _segment_cpu.py) with the
'atom_virial' buffer kind: the per-atom virial of a rank's owned and ghost
rows from its fp64 edge gradients, so the gloo tests can check the driver's
extra reverse exchange (parallel.ParallelE3GNN.evaluate(atom_virial=True))
without a GPU."""
import torch

from _segment_cpu import CpuSegmentEngine
from sevennet_finetuning_amd.model import atom_virial_partition


class CpuVirialSegmentEngine(CpuSegmentEngine):
    def dim(self, kind, t):
        return 6 if kind == 'atom_virial' else super().dim(kind, t)

    def _buf(self, kind, t):
        return self.W if kind == 'atom_virial' else super()._buf(kind, t)

    def atom_virial(self):
        self.W = atom_virial_partition(self.n, self.center, self.nbr, self.vec.detach(), self.dvec)
        return self.W


def make_engine(rg, dtype=torch.float64):
    eng = CpuVirialSegmentEngine(dtype)
    eng._types_local = torch.as_tensor(rg.types[:rg.n_local], dtype=torch.int64)
    return eng
