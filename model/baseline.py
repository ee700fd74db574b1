"""reference model/baseline.py -> sml_amd.baseline: the SPMF / full-retrain / fine-tune baselines and their command line
(`python model/baseline.py --method full|fine|spmf ...` or `python -m model.baseline ...`)."""
import os
import sys

if __name__ == "__main__" and __package__ in (None, ""):       # run as a script: the repository root on the path
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sml_amd.baseline import (SPMF, Reservious, StreamingData, get_parse, main,  # noqa: F401,E402
                              offlineDataset_withsample)

if __name__ == "__main__":
    main()
