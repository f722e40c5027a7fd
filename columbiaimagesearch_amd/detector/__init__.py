"""Detectors of the face path: dlib's HOG face detector on the GPU (hog_detector.py, csrc/hog_detector.hip)."""
from .hog_detector import (FHOGDetectorModel, HOGDetectorHIP, fhog_from_dat, fhog_from_npz, load_fhog_detector, save_npz,  # noqa: F401
                           write_fhog_dat)
