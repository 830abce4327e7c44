"""What kind of input a path names: the drivers' switch between the image and the video branch (the reference keeps a
helper of this name in face_detection_and_extraction/modules/utils/files.py; this is the build's own)."""
import mimetypes

KINDS = ("image", "video")
RAW_MJPEG_EXTENSIONS = (".mjpeg", ".mjpg")     # raw Motion-JPEG streams (modules/utils/video.py): no registered MIME type


def get_file_type(file_src):
    """'camera' for a capture device's index (an int, or a string of digits); 'image' or 'video' by the top-level MIME type of
    the path's extension, with .mjpeg / .mjpg counted as video; None for anything else."""
    name = str(file_src)
    if name.isdigit():
        return "camera"
    if name.lower().endswith(RAW_MJPEG_EXTENSIONS):
        return "video"
    mime, _ = mimetypes.guess_type(name)
    kind = mime.partition("/")[0] if mime else None
    return kind if kind in KINDS else None
