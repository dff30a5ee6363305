"""``model: ctrgcn`` -- CTR-GCN (Chen et al., "Channel-wise Topology Refinement Graph Convolution for Skeleton-Based Action
Recognition", ICCV 2021) on the MI355X kernels.

Constructor ``Model(data_shape={"skeleton": (M, T, V, C)}, num_classes, graph, base_channel=64, adaptive=True, drop_out=0)``, input
(N, M, T, V, C) as ``msg3d`` takes it.  State-dict keys: ``data_bn``, ``l1`` .. ``l10`` with ``gcn1.{PA,alpha}``,
``gcn1.convs.{0,1,2}.conv{1,2,3,4}``, ``gcn1.bn``, ``gcn1.down.{0,1}`` (where the width changes), ``tcn1.branches.*`` (MS-G3D's
MultiScale_TemporalConv with five taps and dilations 1, 2) and ``residual.{conv,bn}`` (where width or stride changes), ``fc``.

Activations travel channels-last (B, T, V, C) float32.  The graph convolution is one row GEMM for the three conv3, one for the six
conv1 / conv2 on the temporal mean, and ``fops.ctr_aggregate`` (fgcn_ctr.hip): the per-sample, per-channel topology
A' = alpha (conv4(tanh(x1 - x2))) + PA is formed on chip and never written to memory.  Everything raises without the built library
/ off gfx950; there is no eager fallback."""
import math

import numpy as np
import torch
import torch.nn as nn

from ... import fops, ops
from ...block import GroupMeanFunction, LinearFunction, data_bn
from ...util.partition_strategy import GraphPartitionStrategy
from ..msg3d.ms_tcn import MultiScale_TemporalConv, TemporalConv


class CTRGC(nn.Module):
    """The four 1x1 convolutions of one subset (a parameter container: ``unit_gcn`` runs the three subsets' convolutions together)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.rel_channels = ops.ctr_reduction(in_channels)
        self.conv1 = nn.Conv2d(in_channels, self.rel_channels, kernel_size=1)
        self.conv2 = nn.Conv2d(in_channels, self.rel_channels, kernel_size=1)
        self.conv3 = nn.Conv2d(in_channels, out_channels, kernel_size=1)
        self.conv4 = nn.Conv2d(self.rel_channels, out_channels, kernel_size=1)


class unit_gcn(nn.Module):
    """out = relu(bn(sum_k A'_k conv3_k(x)) + down(x)), A'_k = alpha conv4_k(tanh(conv1_k(xm)[u] - conv2_k(xm)[v])) + PA[k]."""

    def __init__(self, in_channels: int, out_channels: int, A: np.ndarray, adaptive: bool = True, residual: bool = True):
        super().__init__()
        self.in_channels, self.out_channels, self.adaptive = in_channels, out_channels, adaptive
        self.num_subset = A.shape[0]
        if self.num_subset != ops.CTR_K:
            raise NotImplementedError(f"the HIP CTR graph convolution takes {ops.CTR_K} subsets, the partition has {self.num_subset}")
        self.convs = nn.ModuleList(CTRGC(in_channels, out_channels) for _ in range(self.num_subset))
        self.bn = nn.BatchNorm2d(out_channels)
        if residual and in_channels != out_channels:
            self.down = nn.Sequential(nn.Conv2d(in_channels, out_channels, 1), nn.BatchNorm2d(out_channels))
        elif residual:
            self.down = lambda x: x
        else:
            self.down = lambda x: None
        pa = torch.from_numpy(A.astype(np.float32))
        if adaptive:
            self.PA = nn.Parameter(pa)
        else:
            self.register_buffer("A", pa, persistent=False)      # no state-dict key, no gradient
        self.alpha = nn.Parameter(torch.zeros(1))
        self._forms = fops.ParamForms()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, V, _ = x.shape
        convs = list(self.convs)
        R = convs[0].rel_channels
        x3, _ = fops.conv_params(x, self._forms, "conv3", [c.conv3.weight for c in convs], [c.conv3.bias for c in convs])      # (B, T, V, 3 C)
        xm = fops.ctr_mean_t(x)
        x12, _ = fops.conv_params(xm.view(B, 1, V, xm.shape[-1]), self._forms, "conv12", [c.conv1.weight for c in convs] + [c.conv2.weight for c in convs],
                                  [c.conv1.bias for c in convs] + [c.conv2.bias for c in convs])                                 # (B, 1, V, 6 R)
        y = fops.ctr_aggregate_convs(x3, x12.view(B, V, 2 * self.num_subset * R), [c.conv4 for c in convs], self.alpha,
                                     self.PA if self.adaptive else self.A)
        part = fops.col_stats(y) if self.bn.training else None       # (the running statistics need no partial sums)
        if isinstance(self.down, nn.Sequential):
            d, dpart = fops.conv_params(x, self._forms, "down", [self.down[0].weight], [self.down[0].bias], stats=self.down[1].training,
                                        zero_bias_grad=self.down[1].training)
            res = fops.bn_act(d, dpart, self.down[1])
        else:
            res = self.down(x)
        return fops.bn_act(y, part, self.bn, res=res, relu=True)


class TCN_GCN_unit(nn.Module):
    """relu(tcn1(gcn1(x)) + residual(x))"""

    def __init__(self, in_channels: int, out_channels: int, A: np.ndarray, stride: int = 1, residual: bool = True, adaptive: bool = True):
        super().__init__()
        self.gcn1 = unit_gcn(in_channels, out_channels, A, adaptive=adaptive)
        self.tcn1 = MultiScale_TemporalConv(out_channels, out_channels, kernel_size=5, stride=stride, dilations=[1, 2], residual=False)
        if not residual:
            self.residual = None                        # relu(tcn1(.) + 0): the temporal module's own closing ReLU
        else:
            self.tcn1.act = nn.Identity()
            if in_channels == out_channels and stride == 1:
                self.residual = lambda x: x
            else:
                self.residual = TemporalConv(in_channels, out_channels, kernel_size=1, stride=stride)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.tcn1(self.gcn1(x))
        if self.residual is None:
            return y
        return fops.add_act(y, self.residual(x), relu=True)


def _init(model: "Model", num_classes: int) -> None:
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out")
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    for m in model.modules():
        if isinstance(m, MultiScale_TemporalConv):
            for bn in m.modules():
                if isinstance(bn, nn.BatchNorm2d):
                    nn.init.normal_(bn.weight, 1.0, 0.02)
        elif isinstance(m, unit_gcn):
            nn.init.constant_(m.bn.weight, 1e-6)
    nn.init.normal_(model.fc.weight, 0, math.sqrt(2.0 / num_classes))


class Model(nn.Module):
    def __init__(self, data_shape, num_classes, graph, base_channel: int = 64, adaptive: bool = True, drop_out: float = 0, **kwargs):
        super().__init__()
        num_persons, _, num_joints, num_channels = data_shape["skeleton"]      # (persons, frames, joints, channels)
        A = GraphPartitionStrategy().get_adjacency_matrix_array(graph)
        b = base_channel
        self.data_bn = nn.BatchNorm1d(num_persons * num_channels * num_joints)
        plan = [(num_channels, b, 1, False)] + [(b, b, 1, True)] * 3 + [(b, 2 * b, 2, True)] + [(2 * b, 2 * b, 1, True)] * 2 \
            + [(2 * b, 4 * b, 2, True)] + [(4 * b, 4 * b, 1, True)] * 2
        for i, (cin, cout, stride, residual) in enumerate(plan, start=1):
            setattr(self, f"l{i}", TCN_GCN_unit(cin, cout, A, stride=stride, residual=residual, adaptive=adaptive))
        self.num_layers = len(plan)
        self.fc = nn.Linear(4 * b, num_classes)
        self.drop_out = fops.FusedDropout(drop_out) if drop_out else None
        _init(self, num_classes)

    def mark_packed_stale(self) -> None:
        """Force the re-pack of every weight form at the next forward (what an optimizer step does through the version counters)."""
        fops.mark_forms_stale(self)

    def prepare_recording(self) -> None:
        """GraphStep hook: the one-launch re-pack plan is built (device tables, an H2D copy) before the step is recorded."""
        fops.mark_forms_stale(self)
        fops.refresh_forms(self)

    def recording_pins(self) -> list:
        """GraphStep hook: the forms and the re-pack plan a recording made now replays."""
        return fops.recording_pins(self)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        N, M, T, V, C = x.size()
        fops.refresh_forms(self)
        h = data_bn(x, self.data_bn)          # BatchNorm1d over (m, v, c) -> channels-last (B, T, V, 4): 3 channels travel as 4 (4th zero)
        with fops.deferred_batch_counters(), fops.zero_pool(self):
            for i in range(1, self.num_layers + 1):
                h = getattr(self, f"l{i}")(h)
        h = GroupMeanFunction.apply(h.reshape(N, -1, h.size(-1)))                     # mean over persons, frames and joints
        if self.drop_out is not None:
            h = self.drop_out(h)
        return LinearFunction.apply(h.contiguous(), self.fc.weight, self.fc.bias)
