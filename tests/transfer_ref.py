"""fp64 restatement of the mixed unpool of appearance transfer and of its index construction (full matrix, part-wise, reversed):
plain loops and an einsum over explicitly gathered operands -- nothing shared with the code under test."""
import torch


def unpool_mix_ref(hard, feat, pose_idx, app_idx):
    """hard [n,...,P], feat [m,P,F], pose_idx [K], app_idx [K,P] -> [K,...,F+P] fp64:
    out[k][..][f] = sum_p hard[pose_idx[k]][..][p] * feat[app_idx[k][p]][p][f], then the hard mask itself."""
    P = hard.shape[-1]
    pose_idx = torch.as_tensor(pose_idx).long().reshape(-1)
    app_idx = torch.as_tensor(app_idx).long().reshape(-1, P)
    h = hard.double().cpu()[pose_idx]
    f = feat.double().cpu()[app_idx, torch.arange(P)[None, :]]          # [K,P,F]
    return torch.cat([torch.einsum("k...p,kpf->k...f", h, f), h], dim=-1)


def full_indices(n, m, P):
    """Row-major n x m matrix; the appearance table holds the m column images."""
    pose, app = [], []
    for i in range(n):
        for j in range(m):
            pose.append(i)
            app.append([j] * P)
    return torch.tensor(pose), torch.tensor(app)


def partwise_indices(n, m, P, parts):
    """Row-major n x m matrix; the appearance table holds the n row images, then the m column images: the listed parts come from
    column image j, every other part from row image i itself."""
    pose, app = [], []
    for i in range(n):
        for j in range(m):
            pose.append(i)
            app.append([n + j if p in parts else i for p in range(P)])
    return torch.tensor(pose), torch.tensor(app)


def reversed_indices(B, P):
    return torch.arange(B), torch.tensor([[B - 1 - k] * P for k in range(B)])
