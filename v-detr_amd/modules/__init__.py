"""The reference's sparse module library (models/modules/: ``common`` and ``resnet_block``) and the squeeze-excite blocks of the
same family (``senet``) on ``vdetr_amd.minkowski``."""
