"""Running mean / variance of a stream of batches (reference:
components/standarize_stream.py:9-46, the parallel-variance update), used by the learners to
standardise rewards and returns.  float32 state on the given device and the reference's
formulas; each update is evaluated in float64 and rounded once."""
import torch


class RunningMeanStd:
    def __init__(self, epsilon=1e-4, shape=(), device="cpu"):
        self.mean = torch.zeros(shape, dtype=torch.float32, device=device)
        self.var = torch.ones(shape, dtype=torch.float32, device=device)
        self.count = epsilon

    def update(self, arr):
        # float64 moments: torch's CPU reductions of a float32 tensor accumulate in float64
        # too, the device's float32 tree sums do not
        arr = arr.reshape(-1, arr.size(-1)).double()
        self.update_from_moments(torch.mean(arr, dim=0), torch.var(arr, dim=0), arr.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        # In float32 on the device `tensor / python_number` is a multiplication by the rounded
        # reciprocal, an ulp off the division the CPU performs; an offset in the variance
        # moves every standardised target the same way, so the update runs in float64.
        mean, var = self.mean.double(), self.var.double()
        delta = batch_mean.double() - mean
        tot_count = self.count + batch_count
        new_mean = mean + delta * batch_count / tot_count
        m_a = var * self.count
        m_b = batch_var.double() * batch_count
        m_2 = m_a + m_b + torch.square(delta) * self.count * batch_count / (self.count + batch_count)
        self.mean = new_mean.float()
        self.var = (m_2 / (self.count + batch_count)).float()
        self.count = batch_count + self.count
