from .base import DummyDataset, TrainDataModule, UwUBaseDataset  # noqa: F401
from .text_image_local import LocalTextImageTrainDataset  # noqa: F401
