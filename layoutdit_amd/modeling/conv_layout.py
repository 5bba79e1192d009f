"""Weight re-layouts shared by the convolution backward passes of the FPN (``dit_fpn.py``) and of the RPN head (``rpn.py``)."""
import torch


def _flip_ihwo(w: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 weight -> the operand of its dgrad convolution: [Cin, 3, 3, Cout] with the taps flipped."""
    return w.detach().flip(2, 3).permute(1, 2, 3, 0).contiguous()
