import torch
from .inits import reset  # noqa


def _pool(x, batch, size, mean):
    size = int(batch.max().item() + 1) if size is None else int(size)
    out = torch.zeros(size, x.size(-1), dtype=x.dtype, device=x.device)
    out.index_add_(0, batch, x)
    if mean:
        cnt = torch.zeros(size, dtype=x.dtype, device=x.device)
        cnt.index_add_(0, batch, torch.ones_like(batch, dtype=x.dtype))
        out = out / cnt.clamp(min=1).unsqueeze(-1)
    return out


def global_add_pool(x, batch, size=None):
    return _pool(x, batch, size, False)


def global_mean_pool(x, batch, size=None):
    return _pool(x, batch, size, True)


class JumpingKnowledge(torch.nn.Module):
    def __init__(self, mode, channels=None, num_layers=None):
        super().__init__()
        self.mode = mode.lower()
        assert self.mode in ['cat', 'max']

    def reset_parameters(self):
        pass

    def forward(self, xs):
        if self.mode == 'cat':
            return torch.cat(xs, dim=-1)
        return torch.stack(xs, dim=-1).max(dim=-1)[0]


class _GINBase(torch.nn.Module):
    """What torch_geometric 1.6.3 documents for GINConv and GINEConv:  out_i = nn((1 + eps) x_i + sum_{j -> i} m_j),
    `edge_index[0]` the source j and `[1]` the target i (flow source_to_target).  `eps` is a Parameter under `train_eps` and a
    buffer otherwise: in the state_dict either way."""

    def __init__(self, nn, eps=0., train_eps=False, **kwargs):
        super().__init__()
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer('eps', torch.Tensor([eps]))
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)
        self.eps.data.fill_(self.initial_eps)

    def _aggregate(self, x, edge_index, messages):
        out = (1 + self.eps) * x
        if edge_index.size(1):
            out = out.index_add(0, edge_index[1], messages)
        return self.nn(out)

    def __repr__(self):
        return f'{self.__class__.__name__}(nn={self.nn})'


class GINConv(_GINBase):
    """m_j = x_j."""

    def forward(self, x, edge_index, size=None):
        return self._aggregate(x, edge_index, x[edge_index[0]])


class GINEConv(_GINBase):
    """m_j = relu(x_j + e_ji), `edge_attr` one row per entry of `edge_index`."""

    def forward(self, x, edge_index, edge_attr=None, size=None):
        return self._aggregate(x, edge_index, torch.relu(x[edge_index[0]] + edge_attr))
