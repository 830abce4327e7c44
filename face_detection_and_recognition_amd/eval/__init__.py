"""Accuracy evaluation drivers (face_detection_and_extraction/eval of the reference)."""
