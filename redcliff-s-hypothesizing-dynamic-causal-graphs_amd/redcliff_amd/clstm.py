"""LSTM / cLSTM modules with the reference's constructors, module tree and state_dict keys
(models/clstm.py): ``networks.<j>.lstm.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}`` and
``networks.<j>.linear.{weight, bias}``.  Network j (an ``nn.LSTM(p, h)`` read out by a 1x1 ``Conv1d``)
alone forecasts series j; GC[j][c] is the L2 norm of column c of its ``weight_ih_l0``."""
import torch
import torch.nn as nn


class LSTM(nn.Module):
    def __init__(self, num_series, hidden):
        super().__init__()
        self.num_series = num_series
        self.hidden = hidden
        self.lstm = nn.LSTM(num_series, hidden, batch_first=True)
        self.lstm.flatten_parameters()
        self.linear = nn.Conv1d(hidden, 1, 1)

    def init_hidden(self, batch):
        """Zero (h, c) on the weights' device (float32, as the reference's)."""
        dev = self.lstm.weight_ih_l0.device
        return (torch.zeros(1, batch, self.hidden, device=dev), torch.zeros(1, batch, self.hidden, device=dev))

    def forward(self, X, hidden=None):
        """X (batch, T, p) -> ((batch, T, 1) forecasts, the cell's final (h, c))."""
        if hidden is None:
            hidden = self.init_hidden(X.shape[0])
        out, hidden = self.lstm(X, hidden)
        return self.linear(out.transpose(2, 1)).transpose(2, 1), hidden


def wavelet_rank_mask(num_chans, num_series):
    """The mask GC(rank_wavelets=True) multiplies by (models/clstm.py:66-84): inside every
    (channel, channel) block of 4 x 4 wavelet bands entry (a, b) is 1.3 ** (2 (1 - a) + 2 (1 - b))."""
    per = num_series // num_chans
    assert per == 4  # as the reference: the ranking is tuned for four bands per channel
    rank = per // 4
    w = torch.tensor([1.3 ** (2. * (rank - 1. * i)) for i in range(per)])
    return torch.outer(w, w).repeat(num_chans, num_chans)


class cLSTM(nn.Module):
    def __init__(self, num_chans, hidden, wavelet_level=None, save_path=None):
        super().__init__()
        self.num_chans = num_chans
        self.wavelet_level = wavelet_level
        if wavelet_level is None:
            self.num_series = num_chans
            self.wavelet_mask = None
        else:
            self.num_series = int(num_chans * (wavelet_level + 1))
            self.wavelet_mask = wavelet_rank_mask(num_chans, self.num_series)
            if torch.cuda.is_available():
                self.wavelet_mask = self.wavelet_mask.to(device="cuda")
        # save_path only places the reference's heat map of the mask, which is not drawn here
        self.networks = nn.ModuleList([LSTM(self.num_series, hidden) for _ in range(self.num_series)])

    def forward(self, X, hidden=None):
        """X (batch, T, p) -> ((batch, T, p) forecasts, the p networks' final hidden states)."""
        if hidden is None:
            hidden = [None] * self.num_series
        outs = [net(X, hidden[j]) for j, net in enumerate(self.networks)]
        return torch.cat([o for o, _ in outs], dim=2), tuple(hd for _, hd in outs)

    def perform_prox_update_on_GC_weights(self, lam, lr):
        """In-place group-lasso proximal step on every network's weight_ih_l0 columns."""
        for net in self.networks:
            W = net.lstm.weight_ih_l0
            norm = torch.norm(W, dim=0, keepdim=True)
            W.data = (W / torch.clamp(norm, min=(lam * lr))) * torch.clamp(norm - (lr * lam), min=0.0)
            net.lstm.flatten_parameters()

    def GC(self, threshold=True, combine_wavelet_representations=False, rank_wavelets=False):
        """(p, p) matrix: entry (i, j) says whether (or, threshold=False, how strongly) series j
        Granger-causes series i."""
        G = torch.stack([torch.norm(net.lstm.weight_ih_l0, dim=0) for net in self.networks])
        if rank_wavelets:
            assert self.wavelet_mask is not None
            G = self.wavelet_mask.to(G.device) * G
        if self.wavelet_level is not None and combine_wavelet_representations:
            # the reference's blocks are wavelet_level wide (not wavelet_level + 1); kept as is
            n, w = self.num_chans, self.wavelet_level
            G = G[:n * w, :n * w].reshape(n, w, n, w).sum(dim=(1, 3))
        if threshold:
            return (G > 0).int()
        return G
