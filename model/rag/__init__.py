"""Import point: the reference keeps its image RAG (retrieval of in-context examples) at model/rag/image_rag.py; this build's lives at the
same path, over medplib_amd/rag.py."""
