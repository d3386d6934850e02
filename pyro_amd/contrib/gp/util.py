"""``conditional`` (the Gaussian conditional every GP model predicts with) and ``train`` (an eager optimisation loop
over a GP module); the signatures of pyro/contrib/gp/util.py."""
import torch

from ...infer import TraceMeanField_ELBO


def conditional(Xnew, X, kernel, f_loc, f_scale_tril=None, Lff=None, full_cov=False, whiten=False, jitter=1e-6):
    """Mean and covariance (``full_cov``) or variance of f(Xnew) given that f(X) ~ N(f_loc, f_scale_tril f_scale_tril^T)
    under the prior GP(0, kernel).

    ``f_loc`` is [..., N] and ``f_scale_tril`` [..., N, N] (None: f(X) is known exactly); with ``whiten`` both
    describe v = Lff^-1 f instead, Lff the Cholesky factor of K(X, X) + jitter I (computed here unless given).  With
    Kfs = K(X, Xnew) and W = (Lff^-1 Kfs)^T: loc = W Lff^-1 f_loc, cov = K(Xnew) - W W^T + (W S)(W S)^T with
    S = Lff^-1 f_scale_tril.  A variance is clamped at 0 before the guide's part is added."""
    N = X.size(0)
    M = Xnew.size(0)
    latent_shape = f_loc.shape[:-1]
    if Lff is None:
        Kff = kernel(X).contiguous()
        Kff.view(-1)[::N + 1] += jitter
        Lff = torch.linalg.cholesky(Kff)
    Kfs = kernel(X, Xnew)
    loc_cols = f_loc.reshape(-1, N).t()                                     # [N, prod(latent_shape)]
    n_loc = loc_cols.size(1)
    scale_cols = None
    if f_scale_tril is not None:
        # [..., N, N] -> [N, N * prod(latent_shape)], the latent dims last
        scale_cols = f_scale_tril.permute(-2, -1, *range(len(latent_shape))).reshape(N, -1)
    if whiten:
        v = loc_cols
        W = torch.linalg.solve_triangular(Lff, Kfs, upper=False).t()
        S = scale_cols
    else:
        stacked = [loc_cols, Kfs] + ([] if scale_cols is None else [scale_cols])
        solved = torch.linalg.solve_triangular(Lff, torch.cat(stacked, dim=1), upper=False)
        v = solved[:, :n_loc]
        W = solved[:, n_loc:n_loc + M].t()
        S = None if scale_cols is None else solved[:, n_loc + M:]
    loc = W.matmul(v).t().reshape(latent_shape + (M,))
    if full_cov:
        cov = kernel(Xnew) - W.matmul(W.t())
    else:
        cov = (kernel(Xnew, diag=True) - W.pow(2).sum(dim=-1)).clamp(min=0)
    if S is not None:
        WS = W.matmul(S).reshape((M, N) + latent_shape)
        WS = WS.permute(list(range(2, WS.dim())) + [0, 1])                   # latent_shape + [M, N]
        cov = cov + (WS.matmul(WS.transpose(-2, -1)) if full_cov else WS.pow(2).sum(dim=-1))
    else:
        cov = cov.expand(latent_shape + ((M, M) if full_cov else (M,)))
    return loc, cov


def train(gpmodule, optimizer=None, loss_fn=None, retain_graph=None, num_steps=1000):
    """``num_steps`` eager steps of ``optimizer`` (a torch optimizer; Adam with lr 0.01 by default) on
    ``loss_fn(gpmodule.model, gpmodule.guide)`` (``TraceMeanField_ELBO().differentiable_loss`` by default); returns the
    list of losses.  Nothing is captured into a graph: a GP step factorises a matrix, which synchronises anyway."""
    if optimizer is None:
        optimizer = torch.optim.Adam(gpmodule.parameters(), lr=0.01)
    if loss_fn is None:
        loss_fn = TraceMeanField_ELBO().differentiable_loss

    def closure():
        optimizer.zero_grad()
        loss = loss_fn(gpmodule.model, gpmodule.guide)
        loss.backward(retain_graph=retain_graph)
        return loss

    losses = []
    for _ in range(num_steps):
        loss = optimizer.step(closure)
        losses.append(loss.item() if isinstance(loss, torch.Tensor) else loss)
    return losses
