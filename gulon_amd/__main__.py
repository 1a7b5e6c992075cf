"""python -m gulon_amd query-words / query (gulon_amd/cli.py)."""
import sys

from .cli import main

if __name__ == "__main__":
    sys.exit(main())
