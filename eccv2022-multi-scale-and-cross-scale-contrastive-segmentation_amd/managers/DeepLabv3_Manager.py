"""forward_step for DeepLabv3: the model returns ``logits`` or ``(logits, proj_features)`` and has no auxiliary head, so
``interm_output`` is always None (reference: managers/DeepLabv3_Manager.py:18-53)."""
import torch

from ..losses import LossWrapper
from .BaseManager import BaseManager


class DeepLabv3Manager(BaseManager):
    def forward_step(self, img, lbl, **kwargs):
        ret = dict()
        skip_mem_update = kwargs.get('skip_mem_update', False)
        proj_features = None
        if isinstance(self.loss, LossWrapper):
            lbl = lbl.long()                      # converted once so that prepare() and forward() see one tensor
            if self.return_features:
                if self.model.training:
                    self.loss.prepare(lbl, ready_event=kwargs.get('label_ready'))     # see HRNet_Manager.forward_step
                output, proj_features = self.model(img.float())
                loss = self.loss(output, lbl, deep_features=proj_features, epoch=self.epoch, skip_mem_update=skip_mem_update)
            else:
                output = self.model(img.float())
                loss = self.loss(output, lbl, epoch=self.epoch)
            if 'individual_losses' in kwargs:
                acc = kwargs['individual_losses']
                for key in self.loss.loss_vals:
                    acc[key] += self.loss.loss_vals[key]
                ret['individual_losses'] = acc
        else:
            output = self.model(img.float())
            loss = self.loss(output, lbl.long())
        ret.update(output=output, interm_output=None, feats=proj_features, loss=loss)
        if self.empty_cache:
            torch.cuda.empty_cache()
        return ret
