"""``model: shiftgcn`` -- Shift-GCN (Cheng et al., "Skeleton-Based Action Recognition with Shift Graph Convolutional Network", CVPR 2020)
on the MI355X kernels.

Constructor ``Model(data_shape={"skeleton": (M, T, V, C)}, num_classes, graph, base_channel=64, drop_out=0)``, input (N, M, T, V, C) as
``ctrgcn`` takes it.  The graph supplies only V: the model has no V x V object, so it takes every graph up to 64 joints.  State-dict keys:
``data_bn``, ``l1`` .. ``l10`` with ``gcn1.{Linear_weight,Linear_bias,Feature_Mask}``, ``gcn1.bn`` (BatchNorm1d over V * Cout columns),
``gcn1.down.{0,1}`` (where the width changes), ``tcn1.{bn,bn2}``, ``tcn1.{shift_in,shift_out}.ypos``, ``tcn1.temporal_linear`` and
``residual.{conv,bn}`` (where width or stride changes), ``fc``.

Differences from the upstream modules: the joint-axis position ``xpos`` of upstream's temporal shift (a parameter the upstream forward
never moves off its initial value) and the two index tables ``shift_in`` / ``shift_out`` of upstream's spatial shift (constants:
(i C + j + j C) mod (V C) and (i C + j - j C) mod (V C)) are not parameters or buffers here; the kernels compute the indices.

Activations travel channels-last (B, T, V, C) float32.  A block is two joint shifts (fgcn_shift.hip) around one row GEMM, a BatchNorm per
(joint, channel) column, two frame shifts around a second row GEMM, and the fused BatchNorm / residual / ReLU passes the other models use.
Everything raises without the built library / off gfx950; there is no eager fallback."""
import math

import torch
import torch.nn as nn

from ... import fops
from ...block import GroupMeanFunction, LinearFunction, data_bn
from ..msg3d.ms_tcn import TemporalConv


class Shift_gcn(nn.Module):
    """out = relu(BN1d_{V Cout}(shift_{-1}(shift_{+1}(x) (tanh(Feature_Mask) + 1) @ Linear_weight + Linear_bias)) + down(x))"""

    def __init__(self, in_channels: int, out_channels: int, num_joints: int):
        super().__init__()
        self.in_channels, self.out_channels, self.num_joints = in_channels, out_channels, num_joints
        self.Linear_weight = nn.Parameter(torch.zeros(in_channels, out_channels))
        self.Linear_bias = nn.Parameter(torch.zeros(1, 1, out_channels))
        self.Feature_Mask = nn.Parameter(torch.zeros(1, num_joints, in_channels))
        self.bn = nn.BatchNorm1d(num_joints * out_channels)
        if in_channels != out_channels:
            self.down = nn.Sequential(nn.Conv2d(in_channels, out_channels, 1), nn.BatchNorm2d(out_channels))
        else:
            self.down = lambda x: x
        self._forms = fops.ParamForms()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, V, _ = x.shape
        N = self.out_channels
        s = fops.joint_shift(x, self.Feature_Mask, 1)
        z = fops.linear_params(s, self._forms, "linear", self.Linear_weight, self.Linear_bias, zero_bias_grad=self.bn.training)
        y = fops.joint_shift(z, None, -1).view(B * T, V * N)
        part = fops.col_stats(y) if self.bn.training else None          # (the running statistics need no partial sums)
        if isinstance(self.down, nn.Sequential):
            d, dpart = fops.conv_params(x, self._forms, "down", [self.down[0].weight], [self.down[0].bias], stats=self.down[1].training,
                                        zero_bias_grad=self.down[1].training)
            res = fops.bn_act(d, dpart, self.down[1])
        else:
            res = x
        return fops.bn_act(y, part, self.bn, res=res.view(B * T, V * N), relu=True).view(B, T, V, N)


class Shift(nn.Module):
    """The per-channel frame positions of one temporal shift (a parameter container: ``Shift_tcn`` runs fops.frame_shift on ``ypos``)"""

    def __init__(self, channels: int):
        super().__init__()
        self.ypos = nn.Parameter(torch.zeros(channels))
        nn.init.uniform_(self.ypos, -1.0, 1.0)


class Shift_tcn(nn.Module):
    """bn2(shift_out(relu(temporal_linear(shift_in(bn(x))))))"""

    def __init__(self, in_channels: int, out_channels: int, stride: int = 1):
        super().__init__()
        self.stride = stride
        self.bn = nn.BatchNorm2d(in_channels)
        self.bn2 = nn.BatchNorm2d(in_channels)
        self.shift_in = Shift(in_channels)
        self.shift_out = Shift(out_channels)
        self.temporal_linear = nn.Conv2d(in_channels, out_channels, 1)
        self._forms = fops.ParamForms()

    def pre_bn2(self, x: torch.Tensor):
        """-> (the second shift's output, its BatchNorm partial sums): ``bn2`` is applied by the caller's fused pass"""
        part = fops.col_stats(x) if self.bn.training else None
        u = fops.frame_shift(fops.bn_act(x, part, self.bn), self.shift_in.ypos)
        h, _ = fops.conv_params(u, self._forms, "temporal_linear", [self.temporal_linear.weight], [self.temporal_linear.bias])
        return fops.frame_shift(h, self.shift_out.ypos, self.stride, relu=True, stats=True) if self.bn2.training else \
            (fops.frame_shift(h, self.shift_out.ypos, self.stride, relu=True), None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        w, part = self.pre_bn2(x)
        return fops.bn_act(w, part, self.bn2)


class TCN_GCN_unit(nn.Module):
    """relu(tcn1(gcn1(x)) + residual(x)); ``tcn1``'s closing BatchNorm, the add and the ReLU are one pass"""

    def __init__(self, in_channels: int, out_channels: int, num_joints: int, stride: int = 1, residual: bool = True):
        super().__init__()
        self.gcn1 = Shift_gcn(in_channels, out_channels, num_joints)
        self.tcn1 = Shift_tcn(out_channels, out_channels, stride=stride)
        if not residual:
            self.residual = None
        elif in_channels == out_channels and stride == 1:
            self.residual = lambda x: x
        else:
            self.residual = TemporalConv(in_channels, out_channels, kernel_size=1, stride=stride)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        w, part = self.tcn1.pre_bn2(self.gcn1(x))
        return fops.bn_act(w, part, self.tcn1.bn2, res=None if self.residual is None else self.residual(x), relu=True)


def _init(model: "Model", num_classes: int) -> None:
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out")
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    for m in model.modules():
        if isinstance(m, Shift_gcn):
            nn.init.normal_(m.Linear_weight, 0, math.sqrt(1.0 / m.out_channels))
            nn.init.constant_(m.Linear_bias, 0)
            nn.init.constant_(m.Feature_Mask, 0)
            nn.init.constant_(m.bn.weight, 1e-6)
    nn.init.normal_(model.fc.weight, 0, math.sqrt(2.0 / num_classes))


class Model(nn.Module):
    def __init__(self, data_shape, num_classes, graph, base_channel: int = 64, drop_out: float = 0, **kwargs):
        super().__init__()
        num_persons, _, num_joints, num_channels = data_shape["skeleton"]      # (persons, frames, joints, channels)
        b = base_channel
        self.data_bn = nn.BatchNorm1d(num_persons * num_channels * num_joints)
        plan = [(num_channels, b, 1, False)] + [(b, b, 1, True)] * 3 + [(b, 2 * b, 2, True)] + [(2 * b, 2 * b, 1, True)] * 2 \
            + [(2 * b, 4 * b, 2, True)] + [(4 * b, 4 * b, 1, True)] * 2
        for i, (cin, cout, stride, residual) in enumerate(plan, start=1):
            setattr(self, f"l{i}", TCN_GCN_unit(cin, cout, num_joints, stride=stride, residual=residual))
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
