"""Measuring and probing tools, run as scripts; a package so that they can share tools/timing.py."""
