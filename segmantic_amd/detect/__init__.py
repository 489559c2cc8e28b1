"""Landmark detection: the vertebra-landmark transforms of the reference's ``segmantic.detect``."""
