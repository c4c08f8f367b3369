"""The reference's sparse module library (models/modules/: ``common`` and ``resnet_block``) on ``vdetr_amd.minkowski``."""
