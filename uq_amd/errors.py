"""The one error class of the package, in a module of its own: `python -m uq_amd.uq` runs uq.py as `__main__`, and a class defined there
would exist a second time for every module that imports uq_amd.uq."""


class UqError(Exception):
    """The reference prints and exit()s (uq.py:48-50); the library form raises, main() prints."""


def error(message):
    raise UqError(message)
