"""Model zoo.  The model classes load lazily: importing the package pulls in no compiler."""
_EXPORTS = {"MobileNetV1Model": "image_classifier", "mobilenet_v1_graph_def": "mobilenet",
            "DeepLabV3Model": "image_classifier", "deeplab_v3_graph_def": "deeplab",
            "UNetModel": "image_classifier", "unet_graph_def": "unet", "export_unet_saved_model": "unet",
            "SSDMobileNetModel": "image_classifier", "ssd_mobilenet_v1_graph_def": "ssd",
            "LSTMClassifierModel": "lstm", "lstm_classifier_graph_def": "lstm",
            "VideoClassifierModel": "c3d", "c3d_graph_def": "c3d", "export_c3d_saved_model": "c3d",
            "KeywordSpotterModel": "speech", "speech_commands_graph_def": "speech",
            "export_keyword_spotter_saved_model": "speech",
            "StyleTransferModel": "style_transfer", "style_transfer_graph_def": "style_transfer",
            "export_style_transfer_saved_model": "style_transfer"}

__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib

        return getattr(importlib.import_module(f"{__name__}.{_EXPORTS[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
