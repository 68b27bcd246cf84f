"""Learning-rate schedules the reference's yaml files name (nablaDFT/schedulers.py): config/model/graphormer3d-small.yaml points its ``lr_scheduler`` at
``get_linear_schedule_with_warmup``."""
from torch.optim.lr_scheduler import LambdaLR


def get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, last_epoch=-1):
    """LambdaLR: linear from 0 to the optimizer's lr over ``num_warmup_steps`` steps, then linear down to 0 at ``num_training_steps``."""
    def factor(step):
        if step < num_warmup_steps:
            return step / max(1, num_warmup_steps)
        return max(0.0, (num_training_steps - step) / max(1, num_training_steps - num_warmup_steps))
    return LambdaLR(optimizer, factor, last_epoch)
