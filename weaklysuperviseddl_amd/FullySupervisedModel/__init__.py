"""Drop-in surface mirroring the reference's ``FullySupervisedModel/``: ``SupervisedModel`` (DeepLabV3-ResNet50 trained on the
Oxford-IIIT Pet ground truth, the upper bound of the weakly-supervised results) over a device-resident dataset
(``PetDataset``)."""
from .SupervisedModel import (initialize_model, get_dataloaders, train_one_epoch, evaluate_model,  # noqa: F401
                              run_supervised_training)
